"""The shape of the CALL, as a caller that is not lbdrn_hip/ops.py may make it (include/lbdrn_hip.h, "Alignment" and the
sentences at each entry point): pointers at their declared minimum alignment and no better, a NULL msb where the header
allows one, idx entries outside the raster, a nominal minibatch longer than the rows there are, and rasters with an axis
beyond 65,536 samples.  tests/test_call_shapes_host.py holds the refusals; here everything the header calls supported runs.

Every placement comparison is exact: the call on buffers that lie `skew` bytes past a multiple of 256 (tests/guarded.py)
against the same call on 256-byte aligned buffers, bit for bit, and the aligned result passes the check
tests/test_gpu_workspace_hygiene.py applies to that entry point -- the cases, shapes, inputs and checks are that file's
(two runs that agree on a wrong answer do not pass).  Guards and const inputs are checked inside each run as there.
One fill (0xA5).  The ids read <entry point>-<kernel family / shape>-least_aligned.

Order: the plain entry points first, the fused kernels last."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import oracle as O
import test_gpu_workspace_hygiene as HY
from guarded import Arena
from lbdrn_hip import _lib, ops
from lbdrn_hip.features import FeatCfg
from test_gpu_fuzz import _params

pytestmark = pytest.mark.gpu
GEN, MFMA = _lib.PATH_GENERIC, _lib.PATH_MFMA
FAST, X16, BG = _lib.EVAL_FAST, _lib.EVAL_X16, _lib.EVAL_BACKGROUND
FILL = 0xA5
byref, L, call, ok, bits_equal = ctypes.byref, HY.L, HY.call, HY.ok, HY.bits_equal

# ---------------------------------------------------------------- least-aligned placement

# lbdrn_hip.h, "Alignment": the minimum per argument, by the name tests/test_gpu_workspace_hygiene.py gives the buffer
SKEW = {"img": 2, "msb": 2, "out": 2, "planes": 2,
        "msb_max": 4, "status": 4, "body": 4, "labels": 4, "features": 4, "x": 4, "t": 4, "y": 4, "dy": 4, "dx": 4, "grads": 4,
        "y_out": 4, "exp_avg": 4, "exp_avg_sq": 4, "loss": 4, "losses": 4, "rowtab": 4, "coltab": 4,
        "idx": 8, "sse": 8, "body_bytes": 8}


def declared_skew(name, train):
    """the least alignment the header allows the argument held in buffer `name`, as an offset from a multiple of 256"""
    base = name.rstrip("0123456789")                 # (the fits of a group carry a number)
    if "workspace" in base or base == "tape":
        return 0                                     # 256: workspaces and the tape stay where they are
    if base.startswith("perm"):
        return 8
    if base == "params":
        return 16 if train else 4                    # lbdrn_train_epoch / _group: 16
    return SKEW[base]                                # KeyError: a buffer nobody has placed


class _SkewedTables(ops.FeatureGeometry):
    """the geometry of a run under least_aligned(): its positional tables re-homed 4 bytes past a multiple of 256"""

    def __init__(self, C, H, W, K, D, msb_max, cfg, device, tables=None):
        super().__init__(C, H, W, K, D, msb_max, cfg, device, tables)
        if self.P:
            self.arena = Arena(device)
            self.tabs = [self.arena.const(t.cpu().numpy(), name, skew=4) for name, t in (("rowtab", self.rowtab), ("coltab", self.coltab))]
            self.c.rowtab, self.c.coltab = (b.data_ptr() for b in self.tabs)
            _SkewedTables.built.append(self)

    built = []


@contextlib.contextmanager
def least_aligned(train):
    """every Arena buffer built inside at its declared minimum, every FeatureGeometry's tables at 4; yields the placed names"""
    placed = {}

    def skew(name):
        placed[name] = declared_skew(name, train)
        return placed[name]

    before, ops.FeatureGeometry = ops.FeatureGeometry, _SkewedTables
    del _SkewedTables.built[:]
    try:
        with guarded.placement(skew):
            yield placed
        for g in _SkewedTables.built:       # (the cases with tables name them in must_place: a run that reached the class some
            g.arena.check()                 #  other way than as ops.FeatureGeometry would leave them out and fail there)
            placed.update({b.name: b.skew for b in g.tabs})
    finally:
        ops.FeatureGeometry = before
        del _SkewedTables.built[:]


BY_ID = {c.id: c for c in HY.CASES}


def hygiene(entry, family):
    return BY_ID[f"{entry}-{family}"]


def placement_param(case, train=False, must_place=()):
    return pytest.param(case, train, tuple(must_place), id=case.id + "-least_aligned")


def run_placed(dev, case, train, must_place):
    aligned = case.run(dev, FILL)
    case.check(dev, aligned)
    with least_aligned(train) as placed:
        skewed = case.run(dev, FILL)
    assert placed and any(placed.values()), placed
    for name in must_place:
        assert placed.get(name), (name, placed)
    diff = HY.first_difference(aligned, skewed)
    assert diff is None, f"{case.id}: the result depends on where the caller's buffers lie ({placed}): {diff}"


def randperm_two_seeds():
    seeds, n = [19920517, 3], 1000

    def run(dev, fill):
        A = Arena(dev)
        perm = HY.run_randperm(dev, A, fill, seeds, n)
        A.check()
        return {"perm": perm}

    def check(dev, outs):
        for c, seed in enumerate(seeds):
            assert np.array_equal(outs["perm"][c], HY.torch_randperm(seed, n)), seed
    c = HY.Case("lbdrn_randperm", "one_segment_linked_lists_n1000_two_seeds", run, check)
    return c


PLAIN = [placement_param(hygiene("lbdrn_split_bits", "C1_7x13_msb"), must_place=("img", "msb", "msb_max")),
         placement_param(hygiene("lbdrn_split_bits", "C5_9x31_max_only"), must_place=("img", "msb_max")),
         placement_param(hygiene("lbdrn_labels", "C1_7x13_idx"), must_place=("img", "idx", "labels")),
         placement_param(hygiene("lbdrn_labels", "C5_9x31_raster")),
         # positional tables (coordinates, and the embedding's 25 columns per axis), by index and in raster order
         placement_param(hygiene("lbdrn_features", "C1_D3_9x31_embedding_idx"), must_place=("msb", "idx", "features", "rowtab", "coltab")),
         placement_param(hygiene("lbdrn_features", "C5_D3_9x31_coords_raster"), must_place=("msb", "features", "rowtab", "coltab")),
         placement_param(hygiene("lbdrn_features", "C5_D3_9x31_relative_raster"))]
for _s in HY.NET_SHAPES:
    _f = HY.net_family(*_s)
    PLAIN += [placement_param(hygiene("lbdrn_forward", _f), must_place=("params", "x", "y")),
              placement_param(hygiene("lbdrn_forward_tape", _f)),
              placement_param(hygiene("lbdrn_backward", _f + "_dx"), must_place=("params", "x", "y", "dy", "grads", "dx")),
              placement_param(hygiene("lbdrn_train_step", _f), must_place=("x", "t", "params", "exp_avg", "exp_avg_sq", "loss", "grads"))]
PLAIN += [placement_param(randperm_two_seeds(), must_place=("perm_n1000",)),
          placement_param(hygiene("lbdrn_plane_encode", "noise_16_bit"), must_place=("planes", "body", "body_bytes")),
          placement_param(hygiene("lbdrn_plane_decode", "noise_16_bit"), must_place=("planes", "body", "status"))]


@pytest.mark.parametrize("case,train,must_place", PLAIN)
def test_plain_entry_points_at_their_least_aligned_placement(dev, case, train, must_place):
    run_placed(dev, case, train, must_place)


def test_the_positional_tables_were_moved_too(dev):
    """least_aligned() re-homes a geometry's tables: a run with P > 0 hands the library tables 4 bytes past a multiple of 256"""
    cfg = HY.make_cfg((1, 1, 1, 0))
    with least_aligned(False):
        g = ops.FeatureGeometry(1, 9, 31, 5, 3, 100, cfg, dev)
        assert g.c.P == 25 and g.c.rowtab % 256 == 4 and g.c.coltab % 256 == 4
        assert np.array_equal(g.tabs[0].numpy(np.float32), g.rowtab.cpu().numpy().reshape(-1))
    g = ops.FeatureGeometry(1, 9, 31, 5, 3, 100, cfg, dev)
    assert ops.FeatureGeometry is not _SkewedTables and g.c.rowtab == g.rowtab.data_ptr()      # and nothing stays behind


# ---------------------------------------------------------------- lbdrn_split_bits: *msb_max is a running maximum

@pytest.mark.parametrize("preset", ("above", "below", "equal"))
def test_split_bits_only_raises_the_running_maximum(dev, preset):
    C, H, W = 5, 9, 31
    img = HY.small_image(C, C, H, W)
    msb_o, _, mx = O.split_bits(img, HY.K_IMG)
    assert 2 < mx < 60000
    before = {"above": mx + 7, "below": mx - 2, "equal": mx}[preset]
    A = Arena(dev)
    src, msb = A.const(img, "img"), A.buf(img.nbytes, FILL, name="msb")
    cell = A.buf(4, 0x00, name="msb_max").write(np.array([before], np.int32))
    ok(call(dev, L().lbdrn_split_bits, src.ptr, C, H, W, HY.K_IMG, msb.ptr, cell.ptr))
    A.check()
    assert int(cell.numpy(np.int32)[0]) == max(before, mx)
    assert np.array_equal(msb.numpy(np.uint16), msb_o.reshape(-1))


# ---------------------------------------------------------------- idx entries outside the raster are clamped

def test_labels_and_features_clamp_idx_into_the_raster(dev):
    C, H, W, D = 5, 9, 31, 3
    cfg = HY.make_cfg((1, 0, 1, 1))
    img = HY.small_image(23, C, H, W)
    msb_np, lab, mx = O.split_bits(img, HY.K_IMG)
    idx = np.array([-1, 0, H * W - 1, H * W, 2 ** 40], np.int64)
    rows = np.array([0, 0, H * W - 1, H * W - 1, H * W - 1])
    F = cfg.feature_dim(C, D)
    A = Arena(dev)
    geom = ops.FeatureGeometry(C, H, W, HY.K_IMG, D, mx, cfg, dev)
    src, msb, ix = A.const(img, "img"), A.const(msb_np, "msb"), A.const(idx, "idx")
    labels, feats = A.buf(len(idx) * C * 4, FILL, name="labels"), A.buf(len(idx) * F * 4, FILL, name="features")
    ok(call(dev, L().lbdrn_labels, src.ptr, C, H, W, HY.K_IMG, ix.ptr, len(idx), labels.ptr))
    ok(call(dev, L().lbdrn_features, byref(geom.c), msb.ptr, ix.ptr, len(idx), feats.ptr))
    A.check()
    want_f = O.features(msb_np, D, HY.ocfg_of(cfg), mx)
    assert bits_equal(labels.numpy(np.float32), np.ascontiguousarray(lab[rows], np.float32).reshape(-1))
    assert bits_equal(feats.numpy(np.float32), np.ascontiguousarray(want_f[rows], np.float32).reshape(-1))
    assert not bits_equal(want_f[0], want_f[H * W - 1])      # (the two ends differ: a clamp to the wrong end would show)


# ================================================================ the fused kernels

FUSED_APPLY = [s for s in HY.APPLY_SHAPES if s[1] == MFMA]
FAST_FLAGS = [("fast", FAST), ("fast_x16", FAST | X16), ("fast_background", FAST | BG)]


def eval_call(dev, ins, shape, path, word, with_msb, sse_fill=FILL):
    cfg, img, msb_np, lab, mx, F, pn, net = ins
    C, H, W = shape
    A = Arena(dev)
    geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, cfg, dev)
    src, p = A.const(img, "img"), A.const(pn, "params")
    msb = A.const(msb_np, "msb") if with_msb else None
    sse = A.buf(8, sse_fill, name="sse")
    nws = L().lbdrn_apply_workspace(byref(geom.c), byref(net))
    ws = A.buf(nws, FILL, name="workspace")
    rc = call(dev, L().lbdrn_eval_sse, byref(geom.c), byref(net), src.ptr, msb.ptr if msb else None, p.ptr, sse.ptr, ws.ptr, nws, path | word)
    A.check()
    return rc, sse.numpy(np.float64)


@pytest.mark.parametrize("flag_name,flags", FAST_FLAGS, ids=[f[0] for f in FAST_FLAGS])
@pytest.mark.parametrize("family,path,bc,shape", FUSED_APPLY, ids=[s[0] for s in FUSED_APPLY])
def test_eval_sse_with_a_null_msb_is_the_call_with_the_plane(dev, family, path, bc, shape, flag_name, flags):
    """lbdrn_hip.h at LBDRN_EVAL_FAST: where a fast instance serves the call msb is not read -- NULL gives the sum of the call
    with msb = img >> K bit for bit (itself within 1e-6 of the canonical sum, which is the oracle's) --, and where a canonical
    instance serves it (bc = 128 on one band: no fast instance at four hidden tiles) NULL is refused and *sse is left alone"""
    ins = HY.apply_inputs(bc, shape)
    cfg, img, msb_np, lab, mx, F, pn, net = ins
    assert shape[0] <= 8 and np.array_equal(msb_np, img >> 5)
    rc, with_plane = eval_call(dev, ins, shape, path, flags, True)
    ok(rc)
    rc0, canon = eval_call(dev, ins, shape, path, 0, True)
    ok(rc0)
    sse_o = O.eval_sse(msb_np, lab, 2, HY.ocfg_of(cfg), pn, bc, 2, mx)
    assert abs(float(canon[0]) - sse_o) <= 1e-11 * max(1.0, abs(sse_o)), (canon, sse_o)
    assert abs(float(with_plane[0]) - float(canon[0])) <= 1e-6 * float(canon[0]), (with_plane, canon)
    rc, null = eval_call(dev, ins, shape, path, flags, False)
    if bc == 128:
        assert rc == _lib.E_ARG and b"canonical instance" in L().lbdrn_last_error()
        assert np.array_equal(null.view(np.uint8), np.full(8, FILL, np.uint8))
        return
    ok(rc)
    assert bits_equal(null, with_plane), (null, with_plane)
    if flags == FAST:       # and not by way of the flagless pass: at these shapes the fast sum is another number
        assert not bits_equal(with_plane, canon)


def test_eval_sse_overwrites_sse(dev):
    """lbdrn_hip.h: *sse is overwritten on every path -- the same bits over a zero, a NaN and a large finite value"""
    for family, path, bc, shape in (HY.APPLY_SHAPES[0], HY.APPLY_SHAPES[2], HY.APPLY_SHAPES[4]):
        ins = HY.apply_inputs(bc, shape)
        got = []
        for fill in (0x00, 0xFF, 0x7E):
            rc, sse = eval_call(dev, ins, shape, path, 0, True, sse_fill=fill)
            ok(rc)
            got.append(sse)
        assert bits_equal(got[0], got[1]) and bits_equal(got[0], got[2]) and float(got[0][0]) > 0, (family, got)


FUSED = []
for _fam, _path, _bc, _shape in HY.APPLY_SHAPES:
    _C, _H, _W = _shape
    FUSED.append(placement_param(hygiene("lbdrn_decode_fused", f"{_fam}_{_C}x{_H}x{_W}_y_out"), must_place=("msb", "params", "out", "y_out")))
    for _fn, _fl in HY.EVAL_FLAGS:
        FUSED.append(placement_param(hygiene("lbdrn_eval_sse", f"{_fam}_{_C}x{_H}x{_W}_{_fn}"), must_place=("img", "msb", "params", "sse")))
# prepare + epochs of three steps, the last one ragged: k_train_stream, k_train_split (64 indices by one 16-byte request a lane
# pair; the wide window's ring takes them 4 bytes a lane), the nl = 3 tile kernel, k_train_half at bc = 128, the generic step
TRAIN_PLACED = ("img", "msb", "perm", "params", "exp_avg", "exp_avg_sq", "losses")
for _fam in ("generic_F100", "k_train_stream_LQ24_nl1", "k_train_stream_LQ52", "k_train_stream_split_LQ24_alone", "k_train_split_wide_window_C6",
             "k_train_nl3", "k_train_half_k_dw_wide_bc128_nl1_3_workgroups"):
    FUSED.append(placement_param(hygiene("lbdrn_train_epoch", _fam), train=True, must_place=TRAIN_PLACED))
FUSED.append(placement_param(hygiene("lbdrn_train_epoch_group", "k_train_stream_LQ48_group_of_2"), train=True,
                             must_place=[n + k for n in TRAIN_PLACED for k in "01"]))


@pytest.mark.parametrize("case,train,must_place", FUSED)
def test_fused_entry_points_at_their_least_aligned_placement(dev, case, train, must_place):
    run_placed(dev, case, train, must_place)


# ---------------------------------------------------------------- a nominal minibatch longer than the rows there are

@pytest.mark.parametrize("path", (MFMA, GEN), ids=("fused", "generic"))
def test_a_batch_size_beyond_n_steps_the_one_minibatch_there_is(dev, path):
    """lbdrn_hip.h at batch_size: with n rows and batch_size >= n an epoch is ONE minibatch of n rows, whatever the nominal
    size -- batch_size = n + 1 and 10^4 on a 9 x 12 raster at the headline network give the parameters, moments and loss of
    batch_size = n bit for bit, and LBDRN_PATH_MFMA takes them.  (The workspace is sized for the nominal rows: the header tells a
    caller with -bs beyond its n to pass min(bs, n), and this is why it may.)"""
    shape = (8, 9, 12, 5, 2, 2, HY.REL)
    n = 9 * 12
    cfg, img, msb, lab, mx, F, p0, perm, net = HY.train_inputs(shape, 64, "sine", n)
    outs = {}
    for bs in (n, n + 1, 10 ** 4):
        A = Arena(dev)
        fit = HY.Fit(A, dev, FILL, shape, cfg, img, msb, mx, p0, perm, net, bs)
        assert fit.steps == 1
        fit.prepare(dev, path)
        fit.epoch(dev, 0, path)
        A.check()
        outs[bs] = fit.outs()
    assert np.isfinite(outs[n]["params"]).all() and np.abs(outs[n]["exp_avg"]).max() > 0 and float(outs[n]["losses"][0]) > 0
    for bs in (n + 1, 10 ** 4):
        diff = HY.first_difference(outs[n], outs[bs])
        assert diff is None, (bs, diff)


# ---------------------------------------------------------------- an axis beyond 65,536 samples

LONG = [(2, 70001), (70001, 2)]
LONG_IDS = ["2x70001", "70001x2"]
K_LONG, D_LONG = 5, 2


def noise(seed, C, H, W):
    return np.random.default_rng(seed).integers(0, 65536, (C, H, W)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def long_apply_reference(H, W):
    """C = 1, bc = 32, nl = 2, Sine on uniform 16-bit noise: the oracle's features, raster, outputs and sum, computed once.
    (One band at bc = 32 and not two at 64: the oracle needs 2 s for this raster on a CPU and 6 s for that one.)"""
    C, bc = 1, 32
    cfg = FeatCfg()
    img = noise(H, C, H, W)
    msb, lab, mx = O.split_bits(img, K_LONG)
    F = cfg.feature_dim(C, D_LONG)
    pn = _params(np.random.default_rng(W), F, bc, C, 2, 2.5)
    ocfg = HY.ocfg_of(cfg)
    feats = O.features(msb, D_LONG, ocfg, mx)
    out_o, y_o = O.decode(msb, K_LONG, D_LONG, ocfg, pn, bc, 2, mx, want_y=True)
    sse_o = O.eval_sse(msb, lab, D_LONG, ocfg, pn, bc, 2, mx)
    for a in (img, msb, feats, out_o, y_o, pn):
        a.setflags(write=False)
    return dict(C=C, bc=bc, cfg=cfg, img=img, msb=msb, mx=mx, F=F, pn=pn, feats=feats, out=out_o, y=y_o, sse=sse_o)


@pytest.mark.parametrize("H,W", LONG, ids=LONG_IDS)
def test_long_axis_features_decode_and_eval_equal_the_oracle(dev, H, W):
    """tests/test_gpu_parity.py::test_decode_and_eval_bit_exact_vs_oracle's statement on rasters of 2 x 70001 and 70001 x 2
    (1094 tiles across a row; 70001 tile rows): lbdrn_features in raster order, the raster and the sigmoid outputs of
    lbdrn_decode_fused on both paths bit for bit, the canonical sum within 1e-11, the fast sum within 1e-6 of the canonical"""
    R = long_apply_reference(H, W)
    C, bc, cfg, mx, F = R["C"], R["bc"], R["cfg"], R["mx"], R["F"]
    geom = ops.FeatureGeometry(C, H, W, K_LONG, D_LONG, mx, cfg, dev)
    net = ops.make_net(F, bc, C, 2)
    img_d, msb_d = ops.to_device_u16(R["img"].copy(), dev), ops.to_device_u16(R["msb"].copy(), dev)
    p_d = torch.from_numpy(R["pn"].copy()).to(dev)
    f = ops.features(geom, msb_d).cpu().numpy()
    assert bits_equal(f, R["feats"])
    for path in (GEN, MFMA):
        out, y = ops.decode_fused(geom, net, msb_d, p_d, want_y=True, path=path)
        assert bits_equal(y.cpu().numpy(), R["y"]), path
        assert np.array_equal(ops.from_device_u16(out), R["out"]), path
        sse = float(ops.eval_sse(geom, net, img_d, msb_d, p_d, path=path).item())
        assert abs(sse - R["sse"]) <= 1e-11 * max(1.0, abs(R["sse"])), (path, sse, R["sse"])
    canon = float(ops.eval_sse(geom, net, img_d, msb_d, p_d, path=MFMA).item())
    for kw in (dict(fast=True), dict(fast=True, x16=True), dict(fast=True, background=True)):
        fast = float(ops.eval_sse(geom, net, img_d, msb_d, p_d, path=MFMA, **kw).item())
        assert abs(fast - canon) <= 1e-6 * canon, (kw, fast, canon)


@pytest.mark.parametrize("H,W", LONG, ids=LONG_IDS)
def test_long_axis_fused_epoch_matches_the_generic_step(dev, H, W):
    """C = 2, bc = 64, nl = 2 (F = 50: the streamed step) on the same rasters: lbdrn_train_prepare and one epoch at
    batch_size = 65536 -- three steps, the last of 8930 rows -- within tests/test_gpu_fuzz.py::test_train_fuzz_mfma_matches_generic's
    bounds of the generic step (losses 5e-5 relative; parameters, in rms, within 1 % of the distance three Adam steps travel)"""
    C, bc, nl, bs = 2, 64, 2, 65536
    cfg = FeatCfg()
    img = noise(H + 1, C, H, W)
    msb = img >> K_LONG
    mx = int(msb.max())
    F = cfg.feature_dim(C, D_LONG)
    geom = ops.FeatureGeometry(C, H, W, K_LONG, D_LONG, mx, cfg, dev)
    net = ops.make_net(F, bc, C, nl)
    rng = np.random.default_rng(H)
    p0 = _params(rng, F, bc, C, nl, 1.0)
    perm = torch.from_numpy(rng.permutation(H * W).astype(np.int64)).to(dev)
    nsteps = (H * W + bs - 1) // bs
    assert nsteps == 3 and H * W - 2 * bs == 8930
    img_d, msb_d = ops.to_device_u16(img, dev), ops.to_device_u16(msb, dev)
    out = {}
    for path in (MFMA, GEN):
        p = torch.from_numpy(p0.copy()).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        losses = torch.zeros(nsteps, dtype=torch.float32, device=dev)
        ops.train_epoch(geom, net, img_d, msb_d, perm, bs, p, m, v, 0, 1e-3, losses, path=path)
        out[path] = [t.cpu().numpy() for t in (p, losses)]
    (pa, la), (pb, lb) = out[MFMA], out[GEN]
    np.testing.assert_allclose(la, lb, rtol=5e-5)
    assert np.linalg.norm(pa - pb) <= 0.01 * 1e-3 * nsteps * np.sqrt(len(pa))
    assert np.isfinite(pa).all() and (lb > 0).all() and not np.array_equal(pb, p0)
