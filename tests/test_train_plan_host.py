"""The CPU half of the training-instance census (tests/train_plan_reference.py, tests/train_step_f64.py): the instance lists
and constants of csrc/train_mfma.hip and csrc/train_stream.inc read out of their text, the restatement of the plan held to what
the library tells without a device (lbdrn_train_step_features, lbdrn_train_group_size), every built instance listed exactly
once with a real shape, the instances reached over all (F, C) exactly the built ones, the class boundaries of Fe, the ReLU kink
condition on the inputs of every ReLU row, and the float64 step held to the reference's fixtures.

Nothing here needs a GPU.  tests/test_gpu_train_instances.py steps the table on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_plan_reference as R
import train_step_f64 as T

RTOL_TRAIN = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# constants

def test_constants_are_the_ones_the_source_states():
    k = R.source_constants()
    assert k["STREAM"] == R.STREAM and k["SPLIT"] == R.SPLIT and k["TILE"] == R.TILE
    assert [lq for lq, nl, c in R.STREAM] == sorted(lq for lq, nl, c in R.STREAM)   # make_train_plan takes the first row that holds Fe
    assert R.STREAM_LQ == (16, 24, 32, 48, 52, 64)
    assert R.TILE_LQ == (16, 32, 52) and all(nl == 3 for lq, nl in R.TILE)
    assert k["SPLIT_WIDE_LQ"] == R.SPLIT_WIDE_LQ == 96
    assert k["MAX_GROUP"] == R.MAX_GROUP == 4
    assert k["LDS_BOUND"] == R.LDS_BOUND == 163840
    assert R.STRAIGHT == ((24, 6), (48, 12), (52, 13), (64, 16))
    assert R.SPLIT == ((24, 6), (48, 12), (64, 16), (96, 24)) and dict(R.SPLIT)[R.SPLIT_WIDE_LQ] == 24
    # the streamed list: both layer counts of every LQ on the loop, plus the straight-line ones -- but no 52/2/0, which nothing reaches
    want = sorted([(lq, nl, 0) for lq in R.STREAM_LQ for nl in (1, 2)] + [(lq, 2, nt) for lq, nt in R.STRAIGHT])
    assert sorted(R.STREAM + ((52, 2, 0),)) == want
    for lq, nt in R.STRAIGHT + R.SPLIT:
        assert 16 * nt == 4 * lq                              # a straight-line schedule fills the slots of its LQ
    with open(os.path.join(R.CSRC, "cabi.hip")) as f:
        assert re.findall(r"int lbdrn_train_group_max\(void\) \{ return (\d+); \}", f.read()) == [str(R.MAX_GROUP)]


def test_lds_map_constants_are_the_ones_the_sources_state():
    """stream_lds_floats / tile_lds_floats restate two LDS maps: the pitches and sizes they are made of, as text."""
    with open(os.path.join(R.CSRC, "train_stream.inc")) as f:
        s = f.read()
    with open(R.TRAIN_SOURCE) as f:
        m = f.read()
    for text, want in ((s, ("constexpr int SGP = 260;", "constexpr int SHP = 68, SOP = 20;", "constexpr int SHSZ = WB * SHP + 48;",
                            "constexpr int SZOSZ = WB * SOP + 48;", "constexpr int SZTSZ = TBC_W * WPT;",
                            "constexpr int SRED = 8 + 2 * 64;", "L.idx = total; total += 256;",
                            "const bool alias = 2 * (NST - 1) - 1 >= (SHSZ + SRED + 1023) / 1024 - 1;",
                            "if ((wht + small_floats + h0_extra) * 4 <= 160 * 1024) {")),
                       (m, ("constexpr int TB = 32;", "constexpr int TBC = 64;", "constexpr int HP = 68;", "constexpr int TP = 36;",
                            "constexpr int OP = 20;", "constexpr int WB = 64;", "constexpr int TBC_W = 64;", "constexpr int WPT = 68;"))):
        for line in want:
            assert text.count(line) == 1, line
    # the values DESIGN.md and the comments of train_stream.inc give for the headline maps
    assert R.stream_lds_floats(52, 2) * 4 == 151904 and R.stream_lds_floats(48, 2) * 4 == 147808
    for lq in R.STREAM_LQ:
        for nl in (1, 2):
            assert R.stream_lds_floats(lq, nl) * 4 <= R.LDS_BOUND, (lq, nl)   # what the source's static_assert over the streamed list says


# ---------------------------------------------------------------------------------------------------------------------
# the census

def test_every_reachable_instance_is_listed_exactly_once():
    rows, unreachable = R.census()
    inst_rows = [r for r in rows if r.why == "instance"]
    built = R.built_instances()
    assert len(built) == len(set(built)) == 41
    assert unreachable == ()                                                    # every built instance has a smallest real shape
    listed = [r.inst for r in inst_rows]
    assert len(listed) == len(set(listed)) and set(listed) == set(built)
    assert len({r.id for r in rows}) == len(rows)                               # ids are test ids: unique
    for r in rows:
        s = r.shape
        assert s.C <= 16 and s.D <= 3 and R.H > s.D and R.W > s.D
        assert r.inst == s.instance(alone=r.alone, count=1, B=R.BS) == s.instance(alone=r.alone, count=1, B=R.H * R.W - R.BS)
        if r.why == "instance":   # the smallest: no real shape with fewer multiplied features (then parameters ..) selects it
            smaller = [t for t in R.shapes(s.nl, s.act) if t.size() < s.size()]
            assert all(t.instance(alone=a, count=1, B=2) != r.inst for t in smaller for a in (False, True)), r.id
    # every instance a real shape reaches, over ALL real shapes, is a listed one (nothing reachable was missed)
    reached = {s.instance(alone=a, count=c, B=b) for nl in (1, 2, 3) for act in R.ACTS for s in R.shapes(nl, act)
               for a in (False, True) for c, b in ((1, 1), (1, 2), (1, 100)) if s.plan() is not None}
    assert reached == set(listed)
    print("\n" + R.table_text())


def test_the_instances_reached_over_every_feature_count_are_exactly_the_built_ones():
    """Every (F, C, nl, switches), real shape or not: each steps on a built instance or on the generic kernels (R.instance
    asserts the first), and each built instance is reached -- the lists name nothing that cannot run."""
    # no <52, 2, ., 0>: LQ 52 is Fe 193..208, and all of them have thirteen strips
    assert {(fe + 15) // 16 for fe in range(4 * 48 + 1, 4 * 52 + 1)} == {13}
    seen = set()
    for F in range(1, 420):
        for C in range(1, 17):
            keys = [(True, False, 0, C, 0, F)]                                   # every feature multiplied
            keys += [(True, True, 0, C, D, F) for D in (1, 2, 3) if F == C * (2 * D + 1) ** 2]   # the C window centres skipped
            for key in keys:
                for nl in (1, 2, 3):
                    for act in R.ACTS:
                        for alone in (False, True):
                            for B in (1, 2):
                                seen.add(R.instance(*key, nl, act, alone=alone, count=1, B=B))
    assert seen - {R.GENERIC} == set(R.built_instances())


def _tile_plan_before_the_lists(F, C):
    """The tile kernel's rule at nl = 3 as make_train_plan stated it while LQ 64 was on its list -> (LQ, NT0) or None."""
    RP = (F + C + 3) // 4 * 4
    LQ = next((lq for lq in (16, 32, 52, 64) if F <= 4 * lq and RP <= 4 * lq + 4), 0)
    NT0 = (F + 15) // 16
    if not LQ or 16 * NT0 > 4 * LQ + 4 or R.tile_lds_floats(LQ, NT0, 3) * 4 > R.LDS_BOUND:
        return None
    return LQ, NT0


def test_tile_list_without_lq64_refuses_nothing_it_took():
    """nl = 3, every F <= 256 and C <= 16: the plan never selects LQ 64 and plans exactly what the four-LQ rule planned.  The
    tile kernel's LDS map at LQ 64 is (36,464 + 576 NT0) floats against 40,960: NT0 <= 7, F <= 112, and no such F needs LQ 64."""
    assert R.tile_lds_floats(64, 0, 3) == 36464 and R.tile_lds_floats(64, 1, 3) - R.tile_lds_floats(64, 0, 3) == 576
    planned = 0
    for F in range(1, 257):
        for C in range(1, 17):
            p = R.plan(True, False, 0, C, 0, F, 3, "sine")
            was = _tile_plan_before_the_lists(F, C)
            assert (None if p is None else (p["LQ"], p["NT0"])) == was, (F, C, p, was)
            assert p is None or (p["kind"] == "tile" and p["LQ"] in R.TILE_LQ and p["LQ"] != 64)
            planned += p is not None
    assert planned > 0 and R.plan(True, False, 0, 1, 0, 160, 3, "sine") and not R.plan(True, False, 0, 1, 0, 161, 3, "sine")


def test_plan_restatement_agrees_with_the_library():
    """lbdrn_train_step_features and lbdrn_train_group_size read scalar fields only: for every real shape, both hidden
    activations and one to three hidden layers they say what the restatement says."""
    from lbdrn_hip import _lib
    L = _lib.lib()
    assert L.lbdrn_train_group_max() == R.MAX_GROUP
    checked = 0
    tables = (ctypes.c_float * (256 * 25))()
    for nl in (1, 2, 3):
        for act in R.ACTS:
            for s in R.shapes(nl, act):
                g = _lib.Geom(s.C, R.H, R.W, R.K, s.D, 1, int(s.colors), int(s.relative), s.P, 0, None, None)
                net = _lib.Net(s.F, 64, s.C, nl, 1 if act == "relu" else 0)
                p = s.plan()
                fe = L.lbdrn_train_step_features(ctypes.byref(g), ctypes.byref(net))
                gs = L.lbdrn_train_group_size(ctypes.byref(g), ctypes.byref(net))
                assert fe == (p["Fe"] if p else s.F), (s, fe, p)
                assert gs == (R.MAX_GROUP if R.takes_groups(p) else 1), (s, gs, p)
                # a fused step keeps a row matrix per pixel in its workspace, the generic one nothing that grows with the raster
                ws = []
                for side in (16, 256):
                    g.H = g.W = side
                    g.rowtab = g.coltab = ctypes.addressof(tables) if s.P else None   # (sizing reads no table; it wants them present)
                    ws.append(L.lbdrn_train_workspace(ctypes.byref(g), ctypes.byref(net), 1))
                assert ws[0] > 0 and (ws[1] > ws[0]) == (p is not None), (s, ws, p)
                checked += 1
    assert checked > 1000


def test_class_boundaries_and_strip_fill_are_in_the_table():
    rows, _ = R.census()
    fes = {r.Fe for r in rows if r.inst[0] != "tile" and r.shape.nl == 2}
    reach = R.reachable_fe(2)
    for lo, hi in R.BOUNDARIES:
        below, above = max(f for f in reach if f <= lo), min(f for f in reach if f >= hi)
        assert below in fes and above in fes, (lo, hi, below, above)
        s_lo = next(r for r in rows if r.Fe == below and r.shape.nl == 2 and r.inst[0] != "tile")
        s_hi = next(r for r in rows if r.Fe == above and r.shape.nl == 2 and r.inst[0] != "tile")
        assert s_lo.LQ < s_hi.LQ                              # the two sides step on different classes
    assert [max(f for f in reach if f <= lo) for lo, _ in R.BOUNDARIES] == [64, 96, 128, 192, 202]
    assert [min(f for f in reach if f >= hi) for _, hi in R.BOUNDARIES] == [65, 98, 130, 194, 216]
    for lq in R.STREAM_LQ + (R.SPLIT_WIDE_LQ,):
        of_lq = [r.Fe for r in rows if r.LQ == lq and r.inst[0] != "tile"]
        in_class = [f for f in reach if next(s for s in R.shapes(2, "sine") if s.Fe == f).plan()["LQ"] == lq]
        for full in (True, False):   # a last strip that is full, and one that is not -- wherever a real shape has one
            if any((f % 16 == 0) == full for f in in_class):
                assert any((f % 16 == 0) == full for f in of_lq), (lq, full)
            else:
                assert (lq, full) == (52, True)   # (Fe = 208 = 13 x 16 is no C (2 D + 1)^2 + 2 P - C with C <= 16, D <= 3)
    # the loop schedule at LQ 48 and 64 (NT0 9..11, 14, 15) with a part-filled last strip
    loops = {(r.LQ, r.NT0, r.Fe % 16 != 0) for r in rows if r.inst[0] == "stream" and r.inst[3] == 0 and r.shape.nl == 2}
    assert (48, 9, True) in loops and (64, 14, True) in loops and (64, 15, False) in loops


def test_relu_rows_stay_off_the_kink():
    """Every ReLU row's seed: in the float64 reference of the minibatch that is compared with float64, no hidden
    pre-activation lies within 1e-5 of the layer's largest of 0.  A condition on the inputs; no element is left out of a
    comparison."""
    rows = [r for r in R.census()[0] if r.shape.act == "relu"]
    assert len(rows) >= 18
    for r in rows:
        seed = R.row_seed(r.id)
        x, t, p0, b, loss, g = R.first_step_f64(r.shape, seed)
        assert len(b) == R.BS
        margin = T.kink_margin(p0, x[b], r.shape.F, 64, r.shape.C, r.shape.nl)
        assert margin >= R.KINK, (r.id, seed, margin)
        zs, _, _ = T.forward_f64(p0.astype(np.float64), x[b], r.shape.F, 64, r.shape.C, r.shape.nl, "relu")
        assert all((z > 0).any() and (z < 0).any() for z in zs), r.id     # both sides of the kink are met
        assert np.abs(g).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the float64 step against the reference's fixtures

def _nrel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("case", ("train", "relu_net", "bands4/small"))
def test_f64_step_matches_reference_fixtures(golden, case):
    """tests/train_step_f64.py eats the reference's own teacher-forced runs: loss 1e-5 relative at every step, gradients
    1e-5 norm-relative, parameters 1e-5 (train) / 2e-5 (relu_net, bands4), Adam moments 1e-5 of the largest (train) and the
    project's 2e-5 / 5e-5 (bands4) -- the bounds tests/test_gpu_parity.py, test_gpu_relu.py and test_gpu_autograd.py hold
    the kernels to on the same fixtures."""
    if case == "train":
        G, pre, F, C, act, pb = golden["train"], "", 200, 8, "sine", 1e-5
        x, t, nsteps = G["x"], G["t"], 6
    elif case == "relu_net":
        G, pre, F, C, act, pb = golden["relu_net"], "train/", 200, 8, "relu", 2e-5
        x, t, nsteps = G["x"], G["t"], 3
    else:
        G, pre, F, C, act, pb = golden["bands4"], "small/", 100, 4, "sine", 2e-5
        x, t, nsteps = G["small/features"], G["small/labels"], 6
    get = lambda k: G[pre + k] if pre + k in G.files else None
    lrs = [float(get(f"step{s}/lr")) if get(f"step{s}/lr") is not None else 1e-3 for s in range(nsteps)]
    batches = list(get("batches"))
    assert T.param_count(F, 64, C, 2) == len(get("params0"))
    trace = T.f64_trace(x, t, get("params0"), batches, F, 64, C, lrs, act=act, nl=2)
    for s, (loss, g, p, m, v) in enumerate(trace):
        ref = float(get(f"step{s}/loss"))
        assert abs(loss - ref) <= RTOL_TRAIN * ref, (s, loss, ref)
        if get(f"step{s}/grads") is not None:
            assert _nrel(get(f"step{s}/grads"), g) <= 1e-5, (s, _nrel(get(f"step{s}/grads"), g))
        if get(f"step{s}/params") is not None:
            assert _nrel(get(f"step{s}/params"), p) <= pb, (s, _nrel(get(f"step{s}/params"), p))
    loss, g, p, m, v = trace[-1]
    if get("params_final") is not None:
        assert _nrel(get("params_final"), p) <= pb
    if get("exp_avg") is not None:
        bm, bv = (1e-5, 1e-5) if case == "train" else (2e-5, 5e-5)
        assert np.abs(get("exp_avg") - m).max() <= bm * np.abs(m).max()
        assert np.abs(get("exp_avg_sq") - v).max() <= bv * np.abs(v).max()
    p2, m2, v2 = T.f64_steps(x, t, get("params0"), batches, F, 64, C, lrs, act=act, nl=2)
    assert np.array_equal(p2, p) and np.array_equal(m2, m) and np.array_equal(v2, v)


def test_f64_gradient_is_the_derivative_of_its_loss():
    """nl = 1, 2, 3, both activations: the flat gradient against central differences of the loss, in float64."""
    rng = np.random.default_rng(3)
    F, bc, C, B = 7, 5, 3, 9
    for nl in (1, 2, 3):
        for act in R.ACTS:
            n = T.param_count(F, bc, C, nl)
            p = rng.uniform(-0.3, 0.3, n)
            x, t = rng.uniform(-1, 1, (B, F)), rng.uniform(0, 1, (B, C))
            loss, g = T.loss_and_grad_f64(p, x, t, F, bc, C, nl, act)
            for j in rng.choice(n, 12, replace=False):
                e = np.zeros(n); e[j] = 1e-6
                num = (T.loss_and_grad_f64(p + e, x, t, F, bc, C, nl, act)[0] - T.loss_and_grad_f64(p - e, x, t, F, bc, C, nl, act)[0]) / 2e-6
                assert abs(num - g[j]) <= 1e-6 * max(abs(g).max(), 1e-12) + 1e-9, (nl, act, j, num, g[j])
