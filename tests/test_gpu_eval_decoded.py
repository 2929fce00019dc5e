"""LBDRN_EVAL_DECODED (lbdrn_hip.h) on the GPU: lbdrn_eval_sse's closed-loop sum, the sum over all samples of (img - out)^2 with
out the sample lbdrn_decode_fused writes for the same arguments.

Every comparison here is exact equality of integers.  The expected value is the int64 sum of (img - recon)^2 in numpy, recon
being the ORACLE's reconstruction (oracle.decode) from the same MSB plane and parameters: the existing tests hold
lbdrn_decode_fused to the oracle bit for bit, so this is the sum a decode followed by a compare gives.  All sums here are far
below 2^53, where the header states the float64 result to be the exact integer whatever the summation order.

Every test of this file makes a flagged call, which the library without the flag refuses ("unknown path")."""
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

import apply_plan_reference as R  # noqa: E402
import oracle as O  # noqa: E402
import thin_cases as TC  # noqa: E402
from guarded import FILLS, Arena  # noqa: E402
from lbdrn_hip import _lib, ops  # noqa: E402
from lbdrn_hip.features import FeatCfg  # noqa: E402
from lbdrn_hip.synth import synthetic_tile  # noqa: E402
from test_gpu_fuzz import _params  # noqa: E402

pytestmark = pytest.mark.gpu
AUTO, GEN, MFMA = _lib.PATH_AUTO, _lib.PATH_GENERIC, _lib.PATH_MFMA
FAST, BACKGROUND, VALID, DECODED = _lib.EVAL_FAST, _lib.EVAL_BACKGROUND, _lib.EVAL_VALID, _lib.EVAL_DECODED
K, D, NL = 5, 2, 2


def _bits(x):
    return np.float64(x).tobytes()


class Case:
    """One (image, MSB plane, network) on the device, and the oracle's reconstruction from that plane: made once, left unchanged."""

    def __init__(self, dev, img, params, bc, nl, act="sine", msb=None, k=K, d=D, cfg=None, ocfg=None):
        self.dev, self.img, self.k = dev, img, k
        own, _, _ = O.split_bits(img, k)
        self.msb = own if msb is None else msb
        self.mx = int(self.msb.max())
        C, H, W = img.shape
        cfg = cfg or FeatCfg(activation=act)
        self.geom = ops.FeatureGeometry(C, H, W, k, d, self.mx, cfg, dev)
        self.net = ops.make_net(self.geom.F, bc, C, nl, cfg.act)
        self.params = params
        with O.hidden_activation(act):
            self.recon = O.decode(self.msb, k, d, ocfg or O.FeatCfg(), params, bc, nl, self.mx)
        for a in (self.img, self.msb, self.recon):
            a.setflags(write=False)
        self.img_d = ops.to_device_u16(np.array(img), dev)
        self.msb_d = ops.to_device_u16(np.array(self.msb).astype(np.uint16), dev)
        self.p = torch.from_numpy(np.array(params)).to(dev)
        self.ws = ops.ApplyWorkspace(self.geom, self.net, dev)

    def want(self, V=None):
        d = self.img.astype(np.int64) - self.recon.astype(np.int64)
        keep = np.ones(d.shape, bool) if V is None else self.img != V
        return int((d * d)[keep].sum())

    def call(self, word, reserved=None, start=-1.0):
        """lbdrn_eval_sse with `word` in the case's own workspace -> *sse as a float"""
        out = torch.full((1,), start, dtype=torch.float64, device=self.dev)
        g = _lib.Geom.from_buffer_copy(self.geom.c)
        if reserved is not None:
            g.reserved = reserved
        ops._call(_lib.lib().lbdrn_eval_sse, self.img_d, ctypes.byref(g), ctypes.byref(self.net), ops._ptr(self.img_d), ops._ptr(self.msb_d),
                  ops._ptr(self.p), ops._ptr(out), ops._ptr(self.ws.buf), self.ws.nbytes, word)
        return float(out.item())

    def instance(self, word):
        out = (ctypes.c_int32 * 8)()
        _lib.check(_lib.lib().lbdrn_apply_instance(ctypes.byref(self.geom.c), ctypes.byref(self.net), MFMA | word, out))
        return list(out)


def _exact(got, want):
    assert got == float(want) and int(got) == want, (got, want)


_CASES = {}


def _leg(dev, name):
    """the shapes the nodata-fit tests use: K = 5, D = 2, bc = 64 on 4 x 30 x 41 (ragged both ways), bc = 256 on 8 x 48 x 64"""
    if name not in _CASES:
        (C, H, W), bc = {"bc64": ((4, 30, 41), 64), "bc256": ((8, 48, 64), 256)}[name]
        img = synthetic_tile(7 + C, C, H, W).astype(np.uint16)
        F = FeatCfg().feature_dim(C, D)
        _CASES[name] = Case(dev, img, _params(np.random.default_rng(bc + C), F, bc, C, NL, 2.5), bc, NL)
    return _CASES[name]


# ---------------------------------------------------------------- every serving leg

@pytest.mark.parametrize("name,family", (("bc64", 1), ("bc256", 2)))
def test_every_serving_leg_gives_the_integer(dev, name, family):
    c = _leg(dev, name)
    want = c.want()
    assert 0 < want < 2 ** 53 and np.unique(c.recon & 31).size > 2      # (the outputs move)
    assert c.instance(DECODED)[:4] == c.instance(0)[:4] and c.instance(DECODED)[0] == family and c.instance(DECODED)[3] == 1
    for path in (GEN, MFMA, AUTO):
        for word in (DECODED, DECODED | BACKGROUND):
            got = c.call(path | word)
            print(f"{name} path {path} word {word:#x}: {got!r}, expected {want}")
            _exact(got, want)
    # and it is not the label-space sum
    assert c.call(MFMA) != c.call(MFMA | DECODED)
    for path in (GEN, MFMA):
        with pytest.raises(_lib.LbdrnError) as e:
            c.call(path | DECODED | FAST)
        assert e.value.code == _lib.E_ARG and "canonical" in str(e.value)


# ---------------------------------------------------------------- one evaluation row per family and width

def _eval_rows():
    rows = []
    for r in R.census():
        if r.why == "instance" and r.request == R.EVAL and r.answer.mode == R.EVAL:
            rows.append(r)
    return rows


ROWS = _eval_rows()


def _row_case(dev, row):
    s = row.shape
    img, p = R.row_inputs(row)
    cfg = FeatCfg(s.coords, s.embed, 1.4, R.N_FREQ, s.colors, s.relative, s.act)
    return Case(dev, img, p, s.bc, s.nl, s.act, k=R.K, d=s.D, cfg=cfg, ocfg=R.ocfg(s))


def test_the_rows_cover_every_family_and_width():
    got = {r.inst for r in ROWS}
    assert {("mfma", nt, R.EVAL, act) for nt in (1, 2, 4) for act in R.ACTS} <= got                 # bc 32 / 64 / 128, Sine and ReLU
    assert {(i[0], i[1]) for i in got if i[0] == "wide"} == {("wide", 8), ("wide", 16)}             # bc 128 / 256, Sine


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_evaluation_instance_row(dev, row):
    c = _row_case(dev, row)
    assert c.instance(DECODED) == row.answer.words() == c.instance(0), row.id
    want = c.want()
    got = [c.call(MFMA | DECODED), c.call(MFMA | DECODED | BACKGROUND), c.call(GEN | DECODED)]
    print(f"{row.id}: {got!r}, expected {want}")
    for g in got:
        _exact(g, want)


@pytest.mark.parametrize("fam", ("mfma", "wide"))
def test_more_tiles_than_compute_units(dev, fam):
    """the existing instance test's raster: 3 columns by 16 CUs + 1 rows, so that a virtual workgroup walks more than one tile"""
    cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    row = next(r for r in R.big_rows(cus) if (r.answer.family, r.request) == (fam, R.EVAL))
    c = _row_case(dev, row)
    assert c.instance(DECODED)[7] == cus + 1
    want = c.want()
    for word in (DECODED, DECODED | BACKGROUND):
        _exact(c.call(MFMA | word), want)


# ---------------------------------------------------------------- a plane that is not img >> K, and a dark tile

@pytest.mark.parametrize("bc", (64, 256))
def test_the_difference_is_taken_against_the_plane_given(dev, bc):
    """an all-zero plane under a full-range 16-bit image: out = rint(31 y) <= 31, the differences reach 65535"""
    C, H, W = 4, 30, 41
    img = np.random.default_rng(bc).integers(0, 1 << 16, (C, H, W)).astype(np.uint16)
    img[0, 0, 0], img[C - 1, H - 1, W - 1] = 65535, 65535
    F = FeatCfg().feature_dim(C, D)
    c = Case(dev, img, _params(np.random.default_rng(3 * bc), F, bc, C, NL, 2.5), bc, NL, msb=np.zeros((C, H, W), np.uint16))
    want = c.want()
    assert c.mx == 0 and int(c.recon.max()) <= 31 and want > 2 ** 40
    assert int(np.abs(img.astype(np.int64) - c.recon.astype(np.int64)).max()) >= 65535 - 31
    for path in (GEN, MFMA):
        for word in (DECODED, DECODED | BACKGROUND):
            _exact(c.call(path | word), want)


@pytest.mark.parametrize("C,H,W,Dd", TC.DARK_SHAPES)
def test_a_dark_tile(dev, C, H, W, Dd):
    img = TC.dark_image(C, H, W)
    F = FeatCfg().feature_dim(C, Dd)
    c = Case(dev, img, TC.rand_params(np.random.default_rng([C, H, W]), F, 64, C, NL), 64, NL, d=Dd)
    assert c.mx == 0 and c.geom.c.msb_max == 0
    want = c.want()
    assert want > 0
    for path in (GEN, MFMA):
        _exact(c.call(path | DECODED), want)


# ---------------------------------------------------------------- with LBDRN_EVAL_VALID

@pytest.mark.parametrize("name", ("bc64", "bc256"))
def test_with_the_valid_flag_the_sum_runs_over_the_valid_samples(dev, name):
    base = _leg(dev, name)
    C, H, W = base.img.shape
    holed = np.where(base.img == 1000, 1001, base.img).astype(np.uint16)
    holed[0, 5:20, 3:30] = 1000                    # V in some bands of a pixel only
    holed[:, 22:, 30:] = 1000                      # and in all of them
    c = Case(dev, holed, base.params, base.net.bc, NL)
    absent = int(np.setdiff1d(np.arange(1, 4096), holed)[0])
    for path in (GEN, MFMA):
        for bg in (0, BACKGROUND):
            _exact(c.call(path | DECODED | VALID | bg, reserved=1000), c.want(1000))
            _exact(c.call(path | DECODED | VALID | bg, reserved=absent), c.want())
    assert c.want(1000) < c.want() == c.want(absent)
    void = Case(dev, np.full((C, H, W), 1000, np.uint16), base.params, base.net.bc, NL)
    for path in (GEN, MFMA):
        assert _bits(void.call(path | DECODED | VALID, reserved=1000)) == _bits(0.0)
        _exact(void.call(path | DECODED), void.want())
    assert void.want() > 0


# ---------------------------------------------------------------- workspace and call hygiene

@pytest.mark.parametrize("name,path", (("bc64", MFMA), ("bc256", MFMA), ("bc64", GEN)))
def test_workspace_and_call_hygiene(dev, name, path):
    c = _leg(dev, name)
    want = c.want()
    # *sse is overwritten, whatever it held
    for start in (0.0, float("nan"), 1e300):
        _exact(c.call(path | DECODED, start=start), want)
    # a poisoned workspace and *sse, guard bands around every buffer
    lib = _lib.lib()
    for fill in FILLS:
        A = Arena(dev)
        src, msb, par = A.const(np.array(c.img), "img"), A.const(np.array(c.msb).astype(np.uint16), "msb"), A.const(np.array(c.params), "params")
        sse = A.buf(8, fill, name="sse")
        nws = lib.lbdrn_apply_workspace(ctypes.byref(c.geom.c), ctypes.byref(c.net))
        ws = A.buf(nws, fill, name="workspace")
        with torch.cuda.device(dev):
            rc = lib.lbdrn_eval_sse(ctypes.byref(c.geom.c), ctypes.byref(c.net), src.ptr, msb.ptr, par.ptr, sse.ptr, ws.ptr, nws, path | DECODED,
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.synchronize(dev)
        A.check()
        assert rc == 0
        _exact(float(sse.numpy(np.float64)[0]), want)
    # the same value again, and on a second stream
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = c.call(path | DECODED | BACKGROUND)
    torch.cuda.current_stream(dev).wait_stream(side)
    _exact(other, want)
    _exact(c.call(path | DECODED), want)


@pytest.mark.parametrize("name", ("bc64", "bc256"))
def test_the_other_calls_give_the_bits_they_gave(dev, name):
    """the flagless call, LBDRN_EVAL_FAST and LBDRN_EVAL_VALID, once before and once after a flagged call in the same workspace;
    the flagless sum against the oracle's as tests/test_gpu_apply_instances.py holds it (1e-11 relative)"""
    c = _leg(dev, name)
    V = int(c.img[0, 3, 3])
    words = [(MFMA, None), (MFMA | FAST, None), (MFMA | VALID, V), (GEN, None), (GEN | VALID, V), (MFMA | BACKGROUND, None)]
    before = [c.call(w, reserved=r) for w, r in words]
    _exact(c.call(MFMA | DECODED), c.want())
    _exact(c.call(GEN | DECODED), c.want())
    after = [c.call(w, reserved=r) for w, r in words]
    assert [_bits(x) for x in before] == [_bits(x) for x in after], (before, after)
    _, lab, _ = O.split_bits(c.img, K)
    oracle = O.eval_sse(c.msb, lab, D, O.FeatCfg(), c.params, c.net.bc, NL, c.mx)
    assert abs(before[0] - oracle) <= 1e-11 * oracle and _bits(before[0]) == _bits(before[5])
    assert abs(before[1] - before[0]) <= 1e-6 * before[0] and before[2] < before[0]
