"""The CPU half of the census of the bc = 128 / 256 training step (tests/wide_plan_reference.py): the constants and dispatch
cases of csrc/train_wide.inc read out of its text, every one of the 20 k_train_half and 4 k_dw_wide instances selected by a real
shape and listed exactly once, the reach of the plan over the real feature configurations recomputed from the restatement, the
restatement held to what the library tells without a device (lbdrn_train_step_features, lbdrn_train_group_size,
lbdrn_train_workspace), and the geometry of the minibatches the GPU test steps.

Nothing here needs a GPU.  tests/test_gpu_wide_train_instances.py steps the table on the device."""
import ctypes
import os

import numpy as np

import train_plan_reference as R
import wide_plan_reference as WR


def test_constants_are_the_ones_the_source_states():
    k = WR.source_constants()
    assert k["LQS"] == WR.LQS == (16, 32, 48, 52, 64)
    assert k["WAVE_XP"] == WR.WAVE_XP
    assert (k["DW_KS"], k["HB"], k["WOP"]) == (WR.DW_KS, WR.HB, WR.WOP) == (1024, 32, 16)
    assert (k["GRAD_SLICE"], k["LOSS_BLOCKS"]) == (WR.GRAD_SLICE, WR.LOSS_BLOCKS)
    assert k["LDS_BOUND"] == WR.LDS_BOUND == R.LDS_BOUND
    assert k["HALF_INSTANCES"] == tuple(sorted(WR.HALF_INSTANCES)) and len(set(WR.HALF_INSTANCES)) == 20
    assert sorted(k["DW_INSTANCES"]) == sorted(WR.DW_INSTANCES) and len(set(WR.DW_INSTANCES)) == 4
    assert WR.DW_KS % 256 == 0 and WR.DW_KS // 4 % 64 == 0 and 64 % WR.HB == 0    # a wave's quarter of a slice is whole blocks of 64 rows
    for lq in WR.LQS:
        assert WR.WAVE_XP[lq] >= 4 * lq and WR.WAVE_XP[lq] % 4 == 0       # a row holds the 4 LQ feature slots; the labels need RP <= wave_xp


def test_every_instance_is_reached_and_listed_exactly_once():
    rows, unreachable = WR.census()
    assert unreachable == ()
    first = [r for r in rows if r.why.startswith("instance")]
    assert rows[:len(first)] == tuple(first) and len(first) == 20             # the first block of the table
    assert [r.inst for r in first] == list(WR.HALF_INSTANCES)                   # each exactly once, in the list's order
    assert {r.dw for r in first} == set(WR.DW_INSTANCES)                        # 4 / 4 k_dw_wide
    assert len({r.id for r in rows}) == len(rows)
    for r in rows:
        s = r.shape
        assert s.C <= 16 and s.D <= 3 and WR.H > s.D and WR.W > s.D and s.act == "sine"
        assert WR.instance(s, r.bc) == r.inst
    for r in first:   # the smallest: no real shape that is smaller (Shape.size) selects the instance
        assert all(WR.instance(t, r.bc) != r.inst for t in R.shapes(r.shape.nl, "sine") if t.size() < r.shape.size()), r.id
    for r in rows[len(first):]:
        assert r.bc == 256 and r.shape.nl == 2
    # over ALL real shapes, widths and layer counts: what is reached is what is built
    reached = {WR.instance(s, bc) for bc in WR.BCS for nl in WR.NLS for s in R.shapes(nl, "sine")} - {None}
    assert reached == set(WR.HALF_INSTANCES)
    assert {(i[2], i[1]) for i in reached} == set(WR.DW_INSTANCES)
    print("\n" + WR.table_text())


def test_reach_of_the_plan_over_the_real_feature_configurations():
    """What the plan does with the 361 real feature configurations: five classes, all reached; two shapes pushed to LQ 64 by the
    row pitch and not by Fe <= 4 LQ; nothing with Fe <= 256 refused; NT0 takes every value 1..16."""
    shapes = R.shapes(2, "sine")
    assert len(shapes) == 361
    cls = {}
    for s in shapes:
        p = WR.plan(s, 256)
        assert (p is None) == (s.Fe > 256), s                                   # nothing refused at Fe <= 256
        for bc in WR.BCS:
            for nl in WR.NLS:
                q = WR.plan(R.Shape(s.coords, s.embed, s.colors, s.relative, s.C, s.D, nl, "sine"), bc)
                assert (q is None) == (p is None) and (q is None or (q["LQ"], q["Fe"], q["NT0"]) == (p["LQ"], p["Fe"], p["NT0"]))
        if p:
            cls.setdefault(p["LQ"], []).append((s, p))
    got = {lq: (len(v), min(p["Fe"] for _, p in v), max(p["Fe"] for _, p in v), sorted({p["NT0"] for _, p in v})) for lq, v in cls.items()}
    assert got == {16: (117, 1, 64, [1, 2, 3, 4]), 32: (68, 65, 128, [5, 6, 7, 8]), 48: (39, 130, 192, [9, 10, 11, 12]),
                   52: (9, 194, 200, [13]), 64: (20, 194, 252, [13, 14, 15, 16])}
    # the shapes whose LQ is not the first with Fe <= 4 LQ: the row pitch (features + labels, rounded to 4) decides
    bumped = [(repr(s), p["Fe"], (p["Fe"] + s.C + 3) // 4 * 4, p["LQ"]) for v in cls.values() for s, p in v
              if p["LQ"] != next(lq for lq in WR.LQS if p["Fe"] <= 4 * lq)]
    assert sorted(bumped) == [("C16 D1 cek- F194 nl2 sine", 194, 212, 64), ("C8 D2 c-k- F202 nl2 sine", 202, 212, 64)]
    assert sorted(R.Shape(*c, 2, "sine").key() for c in WR.BUMPED) == sorted(s.key() for v in cls.values() for s, p in v
                                                                               if repr(s) in {b[0] for b in bumped})
    assert WR.reachable_fe()[-1] == 252
    # IM0 = ceil(NT0 / 4) of k_dw_wide: full and part-filled last blocks of four strips
    nt0 = {p["NT0"] for v in cls.values() for _, p in v}
    assert nt0 == set(range(1, 17))


def test_named_rows_are_in_the_table():
    rows, _ = WR.census()
    wide = [r for r in rows if r.bc == 256 and r.shape.nl == 2]
    fes = {r.Fe for r in wide}
    reach = WR.reachable_fe()
    below = [max(f for f in reach if f <= lo) for lo, _ in WR.BOUNDARIES]
    above = [min(f for f in reach if f >= hi) for _, hi in WR.BOUNDARIES]
    assert below == [64, 128, 192, 202] and above == [65, 130, 194, 216]
    assert set(below) | set(above) <= fes
    for (lo, hi), b, a in zip(WR.BOUNDARIES, below, above):
        rb = next(r for r in wide if r.Fe == b and f"boundary {lo}|{hi}, below" in r.why)
        ra = next(r for r in wide if r.Fe == a and f"boundary {lo}|{hi}, above" in r.why)
        assert rb.LQ <= ra.LQ and (rb.LQ < ra.LQ or lo == 208)    # (202 is already on LQ 64: the row pitch, see below)
    for cfg in WR.BUMPED:
        s = R.Shape(*cfg, 2, "sine")
        r = next(r for r in wide if r.shape.key() == s.key() and r.shape.coords == s.coords and r.shape.embed == s.embed)
        assert "row pitch" in r.why and r.LQ == 64 and r.Fe <= 4 * 52 and (r.Fe + s.C + 3) // 4 * 4 == 212 > WR.WAVE_XP[52]
    assert any(r.Fe == 252 and "largest Fe" in r.why and r.NT0 == 16 for r in wide)
    assert {r.NT0 % 4 for r in wide} == {0, 1, 2, 3}
    for lq in WR.LQS:   # a last strip that is full and one that is not, wherever a real shape has one
        in_class = [s.Fe for s in WR.planned_shapes() if WR.plan(s, 256)["LQ"] == lq]
        for full in (True, False):
            if any((f % 16 == 0) == full for f in in_class):
                assert any(r.LQ == lq and (r.Fe % 16 == 0) == full for r in wide), (lq, full)
            else:
                assert (lq, full) == (52, True)                # LQ 52 is Fe 194..200: no multiple of 16
    # k_dw_wide's blocks of four strips: IM0 1..4, the last block full (NT0 = 4, 8, 12, 16) and part-filled
    assert {(r.NT0 + 3) // 4 for r in wide} == {1, 2, 3, 4}
    assert {r.NT0 for r in wide if r.NT0 % 4 == 0} >= {4, 8, 12, 16}
    with open(os.path.join(R.ROOT, "DESIGN.md")) as f:
        assert WR.table_text() in f.read()                     # DESIGN.md 12.1 shows this table


def test_minibatch_geometry_of_the_gpu_cases():
    """The minibatches tests/test_gpu_wide_train_instances.py steps are the ones its docstring says they are."""
    head = R.Shape(*WR.HEADLINE, 2, "sine")
    p = WR.plan(head, 256)
    assert (head.F, p["Fe"], p["LQ"], p["NT0"], p["xo"]) == (200, 192, 48, 12, 192)
    n = WR.H * WR.W
    assert n == 143
    L = lambda B, bc=256, s=head: WR.launches(s, bc, B)
    a, b = L(WR.BS_ODD), L(n - WR.BS_ODD)
    assert (a["nwg"], a["zero_fill"], a["part_workgroup"], a["nrows"]) == (3, True, True, 128) and (b["nwg"], b["zero_fill"], b["nrows"]) == (2, False, 64)
    a, b = L(WR.BS_STALE), L(n - WR.BS_STALE)
    assert (a["nwg"], a["zero_fill"], a["nrows"]) == (4, False, 128) and (b["nwg"], b["zero_fill"], b["nrows"]) == (1, True, 64)
    assert [L(B)["nwg"] for B in (71, 71, 1)] == [3, 3, 1] and n == 2 * WR.BS_TAIL + 1
    big = WR.BIG_H * WR.BIG_W
    assert big == 9312
    a = L(1040)
    assert (a["nwg"], a["zero_fill"], a["nrows"], a["nslices"], a["idle_waves"]) == (33, True, 1088, 2, 3)
    assert big % 1040 == 992 and big // 1040 == 8 and L(992)["nwg"] == 31                 # a short step after eight long ones
    a = L(big)
    assert (a["nwg"], a["nrows"], a["nslices"], a["zero_fill"]) == (291, 9344, 10, True)
    assert a["slices_per_xcd"] == (2, 2, 1, 1, 1, 1, 1, 1) and a["grid"] == 8 * 2 * a["tasks"]
    # tasks per slice: UM IM0 + UM^2 + 1
    assert L(90)["tasks"] == 4 * 3 + 16 + 1 and L(90, 128)["tasks"] == 2 * 3 + 4 + 1
    assert WR.launches(R.Shape(*WR.HEADLINE, 1, "sine"), 256, 90)["tasks"] == 4 * 3 + 1
    for r in WR.census()[0]:
        g = WR.launches(r.shape, r.bc, 90)
        assert g["part_strip_block"] == (r.NT0 % 4 != 0) and g["IM0"] == (r.NT0 + 3) // 4


def test_no_plan_for_relu_three_layers_or_other_widths():
    for cfg in (WR.HEADLINE, (1, 1, 1, 1, 3, 1), (0, 0, 1, 0, 1, 0)):
        for bc in WR.BCS:
            assert WR.plan(R.Shape(*cfg, 2, "relu"), bc) is None and WR.plan(R.Shape(*cfg, 1, "relu"), bc) is None
            assert WR.plan(R.Shape(*cfg, 3, "sine"), bc) is None
            assert WR.plan(R.Shape(*cfg, 2, "sine"), bc) is not None
        for bc in (64, 192, 512):
            assert WR.plan(R.Shape(*cfg, 2, "sine"), bc) is None


def test_plan_restatement_agrees_with_the_library():
    """Through the entry points that read scalar fields only: for every real shape, both widths and one and two hidden layers
    lbdrn_train_step_features says Fe, lbdrn_train_group_size says 1 (the wide step takes one fit per launch), and
    lbdrn_train_workspace says the restated size at minibatches of 1, 33, 1040 and 8192 rows on a small and on a large raster;
    ReLU and three hidden layers at these widths have no fused step: F features and the generic step's workspace."""
    from lbdrn_hip import _lib
    L = _lib.lib()
    tables = (ctypes.c_float * (512 * 25))()
    checked = wide_decides = generic_decides = 0

    def geom(s, side_h, side_w):
        g = _lib.Geom(s.C, side_h, side_w, WR.K, s.D, 1, int(s.colors), int(s.relative), s.P, 0, None, None)
        g.rowtab = g.coltab = ctypes.addressof(tables) if s.P else None          # (sizing reads no table; it wants them present)
        return g

    for bc in WR.BCS:
        for nl in WR.NLS:
            for s in R.shapes(nl, "sine"):
                p = WR.plan(s, bc)
                net = _lib.Net(s.F, bc, s.C, nl, 0)
                g = geom(s, WR.H, WR.W)
                assert L.lbdrn_train_step_features(ctypes.byref(g), ctypes.byref(net)) == (p["Fe"] if p else s.F), (s, bc)
                assert L.lbdrn_train_group_size(ctypes.byref(g), ctypes.byref(net)) == 1, (s, bc)
                for h, w in ((WR.H, WR.W), (512, 512)):
                    g = geom(s, h, w)
                    for bs in (1, 33, 1040, 8192):
                        got = L.lbdrn_train_workspace(ctypes.byref(g), ctypes.byref(net), bs)
                        assert got == WR.workspace_bytes(s, bc, h, w, bs), (s, bc, h, w, bs, got)
                        if p:
                            wd = WR.wide_workspace_bytes(s, bc, h, w, bs) > WR.generic_workspace_bytes(s, bc, bs)
                            wide_decides += wd
                            generic_decides += not wd
                checked += 1
    assert checked == 4 * 361 and wide_decides > 4000 and generic_decides > 0   # the comparison did see wide_ws_layout's total
    for s, bc in ((R.Shape(*WR.HEADLINE, 2, "relu"), 128), (R.Shape(*WR.HEADLINE, 3, "sine"), 256), (R.Shape(*WR.HEADLINE, 1, "relu"), 256)):
        net = _lib.Net(s.F, bc, s.C, s.nl, 1 if s.act == "relu" else 0)
        g = geom(s, WR.H, WR.W)
        assert WR.plan(s, bc) is None
        assert L.lbdrn_train_step_features(ctypes.byref(g), ctypes.byref(net)) == s.F
        assert L.lbdrn_train_group_size(ctypes.byref(g), ctypes.byref(net)) == 1
        assert L.lbdrn_train_workspace(ctypes.byref(g), ctypes.byref(net), 90) == WR.generic_workspace_bytes(s, bc, 90)


def test_zero_lr_epoch_is_the_sum_the_moments_should_hold():
    """zero_lr_epoch_f64 against the closed forms: exp_avg = sum 0.1 0.9^(S-1-s) g_s, exp_avg_sq = sum 0.001 0.999^(S-1-s) g_s^2."""
    s = R.Shape(0, 0, 1, 1, 3, 1, 2, "sine")
    img, p0, perm = WR.fit_inputs(s, 128, 0, 0)
    x, t = WR.features_and_labels_f64(s, img)
    losses, m, v, grads = WR.zero_lr_epoch_f64(s, 128, x, t, p0, perm, 60)
    S = len(grads)
    assert S == 3 and len(losses) == 3
    np.testing.assert_allclose(m, sum(0.1 * 0.9 ** (S - 1 - k) * g for k, g in enumerate(grads)), rtol=0, atol=1e-13 * np.abs(m).max())
    np.testing.assert_allclose(v, sum(0.001 * 0.999 ** (S - 1 - k) * g * g for k, g in enumerate(grads)), rtol=0, atol=1e-13 * np.abs(v).max())
    assert [n for n, _ in WR.blocks(s, 128)] == ["W_0", "b_0", "W_1", "b_1", "W_last", "b_last"]
    assert sum(sl.stop - sl.start for _, sl in WR.blocks(s, 128)) == len(p0)
    mx = {k: int((WR.fit_inputs(s, 128, 0, k)[0] >> WR.K).max()) for k in range(4)}
    assert len(set(mx.values())) == 4                                          # the fits differ in the largest MSB value
