"""Every instance of the fused apply pass run once, by name: the 32 kernels of APPLY_INSTANCES and
WAPPLY_INSTANCES at the smallest real shape that selects each, one row per plan decision, and one raster with more tiles than
the device has compute units per kernel family and mode -- the census of tests/apply_plan_reference.py, which
tests/test_apply_plan_host.py proves complete on the CPU.

Per row, on rasters of a few tiles (17 x 65, 5 x 33, 64 x 64: ragged both ways, fewer rows than a tile, four full tiles), 16-bit
noise at K = 5, weights of mixed magnitude:
  DECODE instances     the raster and y bit for bit the oracle's and LBDRN_PATH_GENERIC's;
  EVAL instances       the sum within 1e-11 relative (tests/test_gpu_fuzz.py) of the oracle's and the generic path's; the same
                       bits on two runs and on the background grid;
  EVAL_FAST / _X16     the sum within the header's 1e-6 relative of a FLOAT64 evaluation of the same float32 parameters and
                       features (the oracle's features, a float64 forward in numpy) and of the canonical sum; the same bits on two
                       runs, on the background grid, with msb NULL and with msb a different plane (a fast instance reads
                       img >> K); a request for the exact-operand pass that a fast instance serves gives the fast request's bits;
  every row            lbdrn_apply_instance names the row's instance for the call just made, LBDRN_PATH_MFMA succeeds, and
                       lbdrn_apply_workspace is the restated size.
What keeps a sum from hiding a wrong tile or channel is a condition on the float64 evaluation, proved on the CPU for every row
(test_no_sum_of_the_census_can_hide_a_wrong_tile_or_two_exchanged_channels) and here again for the rasters sized by the
device's own compute-unit count."""
import ctypes

import numpy as np
import pytest
import torch

import apply_plan_reference as R
import oracle as O
from lbdrn_hip import ops
from lbdrn_hip.features import FeatCfg

pytestmark = pytest.mark.gpu
L = ops._lib
GEN, MFMA = L.PATH_GENERIC, L.PATH_MFMA

ROWS = R.census()
BIG = tuple((fam, mode) for fam, modes in (("mfma", R.REQUESTS), ("wide", R.WIDE_MODES)) for mode in modes)
RAN = {}        # instance -> ids of the rows that ran it
DIST = []       # (row id, serving mode, |sum - float64| / float64, the canonical pass's own)


def _word(request):
    return {R.DECODE: L.APPLY_DECODE, R.EVAL: 0, R.FAST: L.EVAL_FAST, R.X16: L.EVAL_FAST | L.EVAL_X16}[request]


class Device:
    """a row's inputs on the device"""

    def __init__(self, row, dev):
        s, ref = row.shape, R.reference(row)
        self.row, self.ref, self.dev = row, ref, dev
        cfg = FeatCfg(s.coords, s.embed, 1.4, R.N_FREQ, s.colors, s.relative, s.act)
        self.geom = ops.FeatureGeometry(s.C, s.H, s.W, R.K, s.D, ref["mx"], cfg, dev)
        assert (self.geom.F, self.geom.P) == (s.F, s.P)
        self.net = ops.make_net(s.F, s.bc, s.C, s.nl, cfg.act)
        self.img = ops.to_device_u16(ref["img"].copy(), dev)          # (the reference's arrays are read-only; torch wants writable ones)
        self.msb = ops.to_device_u16(ref["msb"].copy(), dev)
        self.p = torch.from_numpy(ref["params"].copy()).to(dev)
        self.ws = ops.ApplyWorkspace(self.geom, self.net, dev)

    def sse(self, request, path=MFMA, background=False, msb="own"):
        """lbdrn_eval_sse with the request's flags; msb: "own", None (NULL) or a tensor"""
        out = torch.full((1,), -1.0, dtype=torch.float64, device=self.dev)
        plane = self.msb if isinstance(msb, str) else msb
        ops._call(L.lib().lbdrn_eval_sse, self.img, ctypes.byref(self.geom.c), ctypes.byref(self.net), ops._ptr(self.img), ops._ptr(plane),
                  ops._ptr(self.p), ops._ptr(out), ops._ptr(self.ws.buf), self.ws.nbytes,
                  path | _word(request) | (L.EVAL_BACKGROUND if background else 0))
        return float(out.item())

    def instance(self, request):
        out = (ctypes.c_int32 * 8)()
        L.check(L.lib().lbdrn_apply_instance(ctypes.byref(self.geom.c), ctypes.byref(self.net), MFMA | _word(request), out))
        return list(out)


def _rel(a, b):
    return abs(a - b) / b


def run_row(row, dev):
    """the checks of the module docstring on one row -> lbdrn_apply_instance's words for it"""
    s, a = row.shape, row.answer
    d = Device(row, dev)
    ref = d.ref
    # 4. the instance is the row's, and the workspace the restated one
    got = d.instance(row.request)
    assert got == a.words(), (row.id, got, a.words())
    fwd = lambda chunk: L.lib().lbdrn_forward_workspace(ctypes.byref(d.net), chunk)
    assert d.ws.nbytes == R.apply_workspace(s, fwd), row.id
    if a.mode == R.DECODE:
        out, y = ops.decode_fused(d.geom, d.net, d.msb, d.p, want_y=True, path=MFMA, ws=d.ws)
        gen, ygen = ops.decode_fused(d.geom, d.net, d.msb, d.p, want_y=True, path=GEN)
        with O.hidden_activation(s.act):
            want, ywant = O.decode(ref["msb"], R.K, s.D, R.ocfg(s), ref["params"], s.bc, s.nl, ref["mx"], want_y=True)
        out, y = ops.from_device_u16(out), y.cpu().numpy()
        bad = np.argwhere(y.view(np.int32).reshape(s.H, s.W, s.C) != ywant.view(np.int32).reshape(s.H, s.W, s.C))
        where = None if not len(bad) else dict(pixel=tuple(bad[0][:2]), channel=int(bad[0][2]), tile=(int(bad[0][0]) // a.TH, int(bad[0][1]) // R.TILE_W), wrong=len(bad))
        assert where is None, (row.id, where)
        assert np.array_equal(out, want), row.id
        assert np.array_equal(ops.from_device_u16(gen), want) and np.array_equal(ygen.cpu().numpy().view(np.int32), ywant.view(np.int32)), row.id
        assert np.unique(want & ((1 << R.K) - 1)).size > 2, row.id          # (the outputs move: not a flat 0.5)
    else:
        canon = [d.sse(R.EVAL), d.sse(R.EVAL), d.sse(R.EVAL, background=True)]
        gen = d.sse(R.EVAL, path=GEN)
        with O.hidden_activation(s.act):
            want = O.eval_sse(ref["msb"], ref["lab"], s.D, R.ocfg(s), ref["params"], s.bc, s.nl, ref["mx"])
        own = _rel(canon[0], ref["sse64"])
        if a.mode == R.EVAL:
            # 2. the canonical sum; a fast request that a canonical instance serves (C > 8, bc = 128) gives the same bits and reads msb
            asked = [d.sse(row.request), d.sse(row.request), d.sse(row.request, background=True)]
            print(f"{row.id}: |canonical - float64| / float64 = {own:.3e}")
            assert canon[0] == canon[1] == canon[2] == asked[0] == asked[1] == asked[2], (row.id, canon, asked)
            assert _rel(canon[0], want) <= 1e-11 and _rel(canon[0], gen) <= 1e-11, (row.id, canon[0], want, gen)
            if R.is_fast(row.request):
                with pytest.raises(L.LbdrnError) as e:
                    d.sse(row.request, msb=None)
                assert e.value.code == L.E_ARG
            DIST.append((row.id, R.EVAL, own, own))
        else:
            # 3. a fast or exact-operand instance
            fast = [d.sse(row.request), d.sse(row.request), d.sse(row.request, background=True)]
            null = d.sse(row.request, msb=None)
            other = d.sse(row.request, msb=d.msb ^ 0x2A5)                  # a deliberately different plane: never read
            dist = _rel(fast[0], ref["sse64"])
            print(f"{row.id}: |{R.MODE_NAMES[a.mode]} - float64| / float64 = {dist:.3e}, the canonical pass's own {own:.3e}, "
                  f"|fast - canonical| / canonical = {_rel(fast[0], canon[0]):.3e}")
            DIST.append((row.id, a.mode, dist, own))
            assert fast[0] == fast[1] == fast[2] == null == other, (row.id, fast, null, other)
            assert _rel(canon[0], want) <= 1e-11 and _rel(canon[0], gen) <= 1e-11 and canon[0] == canon[1] == canon[2], (row.id, canon, want, gen)
            assert dist <= 1e-6, (row.id, fast[0], ref["sse64"])
            assert _rel(fast[0], canon[0]) <= 1e-6, (row.id, fast[0], canon[0])
            if row.request == R.X16 and a.mode == R.FAST:                  # x16 does not qualify: the fast pass's bits
                assert d.instance(R.FAST)[3] == R.FAST and fast[0] == d.sse(R.FAST), row.id
    RAN.setdefault(row.inst, []).append(row.id)
    return got


def _cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_census_row(dev, row):
    run_row(row, dev)


@pytest.mark.parametrize("fam,mode", BIG, ids=[f"{f}-{R.MODE_NAMES[m]}" for f, m in BIG])
def test_more_tiles_than_compute_units(dev, fam, mode):
    """3 columns by 16 CUs + 1 rows, TH = 16: CUs + 1 tiles, so virtual workgroup 0 walks two tiles (a background launch's real
    workgroups two virtual ones each, the first of them three tiles) -- on the device's own compute-unit count, which
    lbdrn_apply_instance's tile count is held against.  The sensitivity condition of the host test, on this raster."""
    cus = _cus(dev)
    row = next(r for r in R.big_rows(cus) if (r.answer.family, r.request) == (fam, mode))
    assert row.answer.tiles == cus + 1 > min(cus, R.MFMA_PARTIALS)
    bound = R.bound_of(row)
    if bound is not None:
        tile, chan = R.sensitivity(row)
        assert tile > 10 * bound and chan > 10 * bound, (row.id, tile, chan)
    assert run_row(row, dev)[7] == cus + 1          # the library's own tile count exceeds the compute units it reports


def test_every_listed_instance_ran(request, capsys):
    """The log of this module names every instance as run, with the rows that ran it, and the distances from float64."""
    selected = {i.callspec.params["row"].id for i in request.session.items
                if getattr(i, "originalname", None) == "test_census_row" and i.module.__name__ == __name__}
    want = {r.inst for r in ROWS if r.id in selected}
    lines = [f"{R.instance_name(inst):44s} ran in {len(RAN.get(inst, []))} rows" for inst in R.built_instances() if inst in want]
    for mode in (R.EVAL, R.FAST, R.X16):
        ds = [(dist, own, rid) for rid, m, dist, own in DIST if m == mode]
        if ds:
            dist, own, rid = max(ds)
            lines.append(f"worst |{R.MODE_NAMES[mode]} - float64| / float64 over {len(ds)} rows: {dist:.3e} ({rid}; the canonical pass there {own:.3e})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    missing = [R.instance_name(i) for i in want if not RAN.get(i)]
    assert not missing, missing
    if len(selected) == len(ROWS):
        assert set(RAN) >= set(R.built_instances()) and len(R.built_instances()) == 32
