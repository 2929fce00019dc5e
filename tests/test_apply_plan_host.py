"""The CPU half of the apply-instance census (tests/apply_plan_reference.py): the lists and constants of csrc/apply_mfma.hip and
csrc/apply_wide.inc read out of their text, the restated planner held to what the library tells without a device
(lbdrn_apply_instance, lbdrn_apply_workspace, the NULL-msb answer of lbdrn_eval_sse) on the census and on a seeded fuzz, every
built instance listed exactly once at its smallest real shape, every plan decision a row of its own, and -- from the float64
evaluation alone -- the condition that keeps a sum from hiding a wrong tile or channel.

Nothing here needs a GPU.  tests/test_gpu_apply_instances.py runs the table on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import apply_plan_reference as R

E_ARG, E_UNSUPPORTED = -1, -3


def _lib():
    from lbdrn_hip import _lib
    return _lib, _lib.lib()


_TABLES = (ctypes.c_float * (8192 * 25))()       # (the host calls read no table; with P > 0 they want them present)


def _structs(s, K=R.K):
    L, _ = _lib()
    tab = ctypes.addressof(_TABLES) if s.P else None
    g = L.Geom(s.C, s.H, s.W, K, s.D, s.msb_max, int(s.colors), int(s.relative), s.P, 0, tab, tab)
    return g, L.Net(s.F, s.bc, s.C, s.nl, R.ACTS.index(s.act))


def _word(request):
    L, _ = _lib()
    return {R.DECODE: L.APPLY_DECODE, R.EVAL: 0, R.FAST: L.EVAL_FAST, R.X16: L.EVAL_FAST | L.EVAL_X16}[request]


def library_answer(s, request, path=2):
    """lbdrn_apply_instance -> (status, out[8] or None)"""
    _, lib = _lib()
    g, net = _structs(s)
    out = (ctypes.c_int32 * 8)(*([-77] * 8))
    rc = lib.lbdrn_apply_instance(ctypes.byref(g), ctypes.byref(net), path | _word(request), out)
    if rc:
        assert list(out) == [-77] * 8            # a refusal leaves out as it was
        return rc, None
    return 0, list(out)


def library_workspace(s):
    _, lib = _lib()
    g, net = _structs(s)
    return lib.lbdrn_apply_workspace(ctypes.byref(g), ctypes.byref(net))


def restated_workspace(s):
    _, lib = _lib()
    _, net = _structs(s)
    return R.apply_workspace(s, lambda chunk: lib.lbdrn_forward_workspace(ctypes.byref(net), chunk))


def null_msb_status(s, request, path=2):
    """lbdrn_eval_sse with msb = NULL and no workspace: E_ARG where something would read msb; where nothing would, the call gets
    past that check and stops at the next one (no device, or the missing workspace) -- nothing is ever launched."""
    _, lib = _lib()
    g, net = _structs(s)
    img, params, sse = (ctypes.c_void_p(0x10000 + 4096 * k) for k in range(3))   # (aligned, never read)
    return lib.lbdrn_eval_sse(ctypes.byref(g), ctypes.byref(net), img, None, params, sse, None, 0, path | _word(request), None)


# ---------------------------------------------------------------------------------------------------------------------
# the text

def test_constants_and_lists_are_the_ones_the_sources_state():
    k = R.source_constants()
    assert k["modes"] == {"MODE_DECODE": R.DECODE, "MODE_EVAL": R.EVAL, "MODE_EVAL_FAST": R.FAST, "MODE_EVAL_X16": R.X16}
    for name in ("APPLY_ROWS", "WAPPLY_ROWS", "WIDE_MODES", "TILE_W", "APPLY_THREADS", "WA_THREADS", "X16_PIECES", "MFMA_PARTIALS",
                 "LDS_RESIDENT", "LDS_WIDE"):
        assert k[name] == getattr(R, name), name
    assert len(R.built_instances()) == len(set(R.built_instances())) == 32
    with open(R.APPLY_SOURCE) as f:
        a = f.read()
    with open(R.WIDE_SOURCE) as f:
        w = f.read()
    # the lines the restatement restates: were one of them to change, the restatement is to be read against it again
    for text, want in ((a, ("q.S0 = g.P + ((q.ncolor + 1) / 2 + 3) / 4 * 4;",
                            "q.pair = fast && q.NT <= 2 && g.use_colors && g.D >= 1 && g.D <= 3 && (g.C % 2) == 0 && q.ncolor == g.C * side * side;",
                            "q.RS = side * side - ((g.relative && g.D > 0) ? 1 : 0);",
                            "if (q.pair) q.S0 = g.P + (g.C / 2) * q.RS;",
                            "q.x16 = x16 && q.pair && g.relative && g.P == 0 && g.msb_max >= 1 && g.msb_max <= 2047 && (q.RS % 8) == 0;",
                            "q.off_w0 = o; o += q.x16 ? (g.C / 2) * q.M16 * X16_PIECES * 64 * q.NT * 4 : q.S0 * 64 * q.NT;",
                            "q.off_ktab = o; o += 2 * 2 * (q.S0 - g.P) + 2;",
                            "q.lds_floats = std::max(o, q.off_rowt + 2 * APPLY_THREADS + 4);",
                            "if (net.C > 32 || net.nl < 1 || net.nl > 15) return false;",
                            "if (make_plan(g, net, &fp, true, false) && (!make_plan(g, net, &xp, true, true) || xp.TH < fp.TH)) mode = MODE_EVAL_FAST;",
                            "if (mode_fast(mode) && net.C > 8) mode = MODE_EVAL;",
                            "if (mode == MODE_EVAL_X16 && !(x16 && apply_row(nt, MODE_EVAL_X16))) mode = MODE_EVAL_FAST;",
                            "if (mode == MODE_EVAL_FAST && !(apply_row(nt, MODE_EVAL_FAST) || wapply_row(nt))) mode = MODE_EVAL;",
                            "A.nvirt = std::min(std::min(A.p.tiles_x * A.p.tiles_y, cus), MFMA_PARTIALS);",
                            "return apply_pack_bytes(g, net) + align_up(MFMA_PARTIALS * sizeof(double), 256) + 256;")),
                       (w, ("q.skip = fast && g.use_colors && g.relative && g.D > 0 && q.ncolor == g.C * q.S2;",
                            "q.G0 = ((q.Fe + 15) / 16 + 1) & ~1;",
                            "if (net.C > 16 || net.nl < 1 || net.nl > 2 || net.F < 1) return false;",
                            "q.off_ktab = o; o += 2 * std::max(q.ncolor, 1) + 2;",
                            "q.lds_floats = std::max(o, q.off_rowt + 2 * WA_THREADS + 4);"))):
        for line in want:
            assert text.count(line) == 1, line
    assert R.FAST_MAX_BANDS == 8 and R.X16_MAX_MSB == 2047
    # serving_mode over its whole domain: the table of DESIGN.md 13, which the source holds by static_assert
    for x in (False, True):
        for nt, want in ((1, (0, 1, 2, 3 if x else 2)), (2, (0, 1, 2, 3 if x else 2)), (4, (0, 1, 1, 1)), (8, (0, 1, 2, 2)), (16, (0, 1, 2, 2))):
            assert tuple(R.serving_mode(m, nt, x) for m in R.REQUESTS) == want, (nt, x)


# ---------------------------------------------------------------------------------------------------------------------
# the census

def test_the_census_names_exactly_the_listed_instances_each_at_its_smallest_real_shape():
    """The 32 instances as tests/test_kernel_disassembly.py reads them out of csrc/apply_mfma.hip; one instance row each; no
    real shape with fewer parameters selects the instance under any request."""
    with open(R.APPLY_SOURCE) as f:
        src = f.read()
    modes = {name: int(v) for name, v in re.findall(r"\b(MODE_[A-Z0-9_]+) = (\d+)", src)}
    rows = [(int(nt), modes[m]) for nt, m in re.findall(r"\bX\((\d+), (MODE_[A-Z0-9_]+)\)", src)]
    wrows = [(int(nt), int(nl)) for nt, nl in re.findall(r"\bX\((\d+), (\d+)\)", src)]
    listed = {("mfma", nt, m, act) for nt, m in rows for act in R.ACTS} | \
             {("wide", nt, nl, m) for nt, nl in wrows for m in (modes["MODE_DECODE"], modes["MODE_EVAL"], modes["MODE_EVAL_FAST"])}
    assert len(listed) == 32
    census = R.census()
    inst = [r for r in census if r.why == "instance"]
    assert len(inst) == 32 and {r.inst for r in inst} == listed
    assert len({r.id for r in census + R.big_rows()}) == len(census) + len(R.big_rows())          # ids are test ids: unique
    assert {r.inst for r in census} == listed                                                     # a variant row runs a listed instance
    smallest = {}
    for req in R.REQUESTS:
        for s in R.real_shapes():
            a = R.resolve(s, req)
            if a is not None:
                smallest.setdefault(a.instance(), s.params())
    assert set(smallest) == listed                                   # over ALL real shapes and requests: nothing else is reached
    for r in inst:
        assert r.shape.params() == smallest[r.inst], r.id
        assert 2 <= r.shape.C <= 32 and 1 <= r.shape.D <= 3
    print("\n" + R.table_text() + "\n" + R.table_text(R.big_rows()).split("\n", 2)[2])


def test_the_examples_of_the_streaming_kernel_select_what_they_are_said_to():
    """bc = 128 with one hidden layer streams only where layer 0 is too large for resident weights (8 bands at D = 3: F = 392);
    with two, the 8-band D = 2 headline features already do; bc = 256 always streams."""
    assert R.resolve(R.Shape(8, 3, 128, 1), R.EVAL).instance() == ("wide", 8, 1, R.EVAL)
    assert R.resolve(R.Shape(8, 2, 128, 1), R.EVAL).instance() == ("mfma", 4, R.EVAL, "sine")
    assert R.resolve(R.Shape(8, 2, 128, 2), R.EVAL).instance() == ("wide", 8, 2, R.EVAL)
    assert R.resolve(R.Shape(8, 3, 128, 1, "relu"), R.EVAL) is None                  # (the streaming kernel is the Sine network's)
    for nl in (1, 2):
        assert R.resolve(R.Shape(2, 1, 256, nl), R.FAST).instance() == ("wide", 16, nl, R.FAST)
    assert R.resolve(R.Shape(2, 1, 96, 1), R.EVAL) is None and R.resolve(R.Shape(2, 1, 256, 3), R.EVAL) is None


VARIANTS = {   # row name -> what the row's plan must show
    "pair-on": lambda s, a: a.pair == 1 and a.mode == R.FAST,
    "pair-off-odd-bands": lambda s, a: a.pair == 0 and a.mode == R.FAST and s.C % 2 == 1 and s.D >= 1 and s.colors,
    "pair-off-D0": lambda s, a: a.pair == 0 and a.mode == R.FAST and s.C % 2 == 0 and s.D == 0 and s.colors,
    "pair-off-no-colours": lambda s, a: a.pair == 0 and a.mode == R.FAST and s.C % 2 == 0 and s.D >= 1 and not s.colors,
    "skip-on": lambda s, a: a.family == "wide" and a.skip == 1 and a.mode == R.FAST,
    "skip-off-absolute": lambda s, a: a.family == "wide" and a.skip == 0 and a.mode == R.FAST and not s.relative and s.D >= 1,
    "skip-off-D0": lambda s, a: a.family == "wide" and a.skip == 0 and a.mode == R.FAST and s.relative and s.D == 0,
    "pad-group": lambda s, a: a.family == "wide" and a.G0 == (a.plan["Fe"] + 15) // 16 + 1,
    "no-pad-group": lambda s, a: a.family == "wide" and a.G0 == (a.plan["Fe"] + 15) // 16,
    "pad-steps": lambda s, a: a.family == "mfma" and 2 * (a.S0 - s.P) - a.plan["ncolor"] in (6, 7),
    "no-pad-steps": lambda s, a: a.family == "mfma" and 2 * (a.S0 - s.P) - a.plan["ncolor"] in (0, 1),
    "x16-M16-1": lambda s, a: a.mode == R.X16 and a.x16 and a.M16 == 1,
    "x16-M16-3": lambda s, a: a.mode == R.X16 and a.x16 and a.M16 == 3,
    "x16-M16-6": lambda s, a: a.mode == R.X16 and a.x16 and a.M16 == 6,
    "x16-to-fast-no-room": lambda s, a: (s.C, s.D, s.bc) == (8, 3, 64) and a.mode == R.FAST and a.pair and not a.x16 and
                           R.make_plan(s, True, True) is None and R.make_plan(s.on(s.H, s.W), True, False)["TH"] == a.TH,
    "x16-to-fast-shorter-tile": lambda s, a: (s.C, s.D, s.bc) == (6, 3, 64) and a.mode == R.FAST and a.pair and not a.x16 and
                                R.make_plan(s, True, True)["x16"] and R.make_plan(s, True, True)["TH"] < a.TH,
    "x16-to-fast-absolute": lambda s, a: a.mode == R.FAST and a.pair and not a.x16 and not s.relative,
    "x16-to-fast-positional": lambda s, a: a.mode == R.FAST and a.pair and not a.x16 and s.relative and s.P > 0,
    "C9-fast-request": lambda s, a: s.C == 9 and a.family == "mfma" and a.mode == R.EVAL and a.pair == 0,
    "C9-x16-request": lambda s, a: s.C == 9 and a.family == "mfma" and a.mode == R.EVAL and a.pair == 0 and a.x16 == 0,
    "bc128-fast-request": lambda s, a: a.family == "mfma" and a.NT == 4 and a.mode == R.EVAL,
    "no-colours-coords-decode": lambda s, a: not s.colors and s.P == 25 and s.F == 50 and a.family == "mfma",
    "no-colours-coords-eval": lambda s, a: not s.colors and s.P == 1 and s.F == 2 and a.family == "mfma",
    "one-band-mfma": lambda s, a: s.C == 1 and a.family == "mfma" and a.mode == R.FAST,
    "one-band-wide": lambda s, a: s.C == 1 and a.family == "wide" and a.mode == R.FAST,
}


def test_every_plan_decision_has_a_row_that_shows_it():
    rows = {r.why: r for r in R.census() if r.why != "instance"}
    for name, shows in VARIANTS.items():
        assert shows(rows[name].shape, rows[name].answer), name
    for fam in ("mfma", "wide"):
        for P in (0, 1, 25):
            r, f = rows[f"P{P}-{fam}"], rows[f"P{P}-{fam}-fast"]
            assert r.shape.P == P and r.answer.family == fam and r.answer.mode == R.DECODE
            assert f.shape.P == P and f.answer.family == fam and f.answer.mode == R.FAST
    th_rows = {name for name in rows if name.startswith("TH")}
    assert set(rows) == set(VARIANTS) | {f"P{P}-{fam}{t}" for P in (0, 1, 25) for fam in ("mfma", "wide") for t in ("", "-fast")} | th_rows
    for name in th_rows:
        th, fam = int(name.split("-")[0][2:]), name.split("-")[1]
        a = rows[name].answer
        assert (a.TH, a.family) == (th, fam) and a.mode == (R.FAST if name.endswith("-fast") else R.EVAL), name
        assert a.tiles_y == (rows[name].shape.H + th - 1) // th
    # instance rows plan whole tiles of 16 rows; the rasters: ragged both ways, fewer rows than a tile, four full tiles
    assert all(r.answer.TH == 16 for r in R.census() if r.why == "instance")
    for fam in ("mfma", "wide"):
        for mode in R.REQUESTS if fam == "mfma" else R.WIDE_MODES:
            met = {(r.shape.H, r.shape.W) for r in R.census() if r.answer.family == fam and r.answer.mode == mode}
            assert met == set(R.RASTERS), (fam, mode, met)


def test_the_tile_heights_that_can_be_planned():
    """Every TH in {16, 8, 4, 2, 1} either has a census row per kernel family or is stated unreachable; k_apply_mfma's fast
    instances meet TH = 16, 8 and 1 only (4 and 2 take more than 8 bands within D <= 3)."""
    reach = R.reachable_th()
    assert reach == {(f, th) for f in ("mfma", "wide") for th in (16, 8, 4, 2, 1)} - set(R.UNREACHABLE_TH)
    have = {(r.answer.family, r.answer.TH) for r in R.census()}
    assert have == reach
    fast_th = {a.TH for req in (R.FAST, R.X16) for s in R.real_shapes() if (a := R.resolve(s, req)) is not None
               and a.family == "mfma" and R.is_fast(a.mode)}
    assert fast_th == {16, 8, 1}
    assert {r.answer.TH for r in R.census() if r.answer.family == "mfma" and R.is_fast(r.answer.mode)} == fast_th
    wide_fast = {r.answer.TH for r in R.census() if r.answer.family == "wide" and r.answer.mode == R.FAST}
    assert wide_fast == {16, 8, 4, 2}
    # within the real shapes (D <= 3) the streaming kernel stops at 4 rows: its TH = 2 rows are the D = 4 ones
    assert {a.TH for s in R.real_shapes() if (a := R.resolve(s, R.EVAL)) is not None and a.family == "wide"} == {16, 8, 4}
    assert all(r.shape.D == 4 for r in R.census() if (r.answer.family, r.answer.TH) == ("wide", 2))
    assert all(r.shape.D <= 3 for r in R.census() if (r.answer.family, r.answer.TH) != ("wide", 2))


def test_design_md_holds_the_census_as_derived():
    """DESIGN.md 13.1 prints the table: the one the restatement derives today, line for line"""
    with open(os.path.join(R.ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert R.table_text() + "\n" + R.table_text(R.big_rows()).split("\n", 2)[2] in text


def test_more_tiles_than_compute_units_rows():
    for cus in (R.CUS, 304, 64):
        rows = R.big_rows(cus)
        assert {(r.answer.family, r.answer.mode) for r in rows} == {("mfma", m) for m in R.REQUESTS} | {("wide", m) for m in R.WIDE_MODES}
        for r in rows:
            assert r.answer.tiles == cus + 1 and r.answer.TH == 16 and (r.shape.H, r.shape.W) == (16 * cus + 1, 3)
    # k_apply_wide at bc = 256 plans TH = 16 from two bands on (the fewest a real shape has), at D = 1 up to 13
    assert [C for C in range(1, 17) if R.make_wapply_plan(R.Shape(C, 1, 256, 1))["TH"] == 16] == list(range(1, 14))


# ---------------------------------------------------------------------------------------------------------------------
# the library

def test_every_census_row_selects_its_instance_in_the_library():
    for r in R.census() + R.big_rows():
        rc, out = library_answer(r.shape, r.request)
        assert rc == 0 and out == r.answer.words(), (r.id, out, r.answer.words())
        assert R.resolve(r.shape, r.request).instance() == r.inst
        assert library_workspace(r.shape) == restated_workspace(r.shape), r.id
        reads = not R.is_fast(r.answer.mode)
        if r.request != R.DECODE:
            assert (null_msb_status(r.shape, r.request) == E_ARG) == reads, r.id


def test_restatement_and_library_agree_on_a_seeded_fuzz():
    """Field for field on 4,000 shapes: 1..33 bands, D 0..4, every feature switch, bc 16..256, 1..4 hidden layers, both
    activations, the four request words on all three paths, msb_max on both sides of 2047 (and 0, which the entry points read as
    1), rasters of 1..300 rows and columns.  Where the restatement has no instance the library answers LBDRN_E_UNSUPPORTED; the
    workspace size is the restated one; msb may be NULL exactly where the restatement says a fast instance serves."""
    L, lib = _lib()
    rng = np.random.default_rng(20261021)
    seen, refused, null_ok = set(), 0, 0
    for it in range(4000):
        coords = bool(rng.integers(0, 2))
        embed = coords and bool(rng.integers(0, 2))
        colors = True if not coords else bool(rng.integers(0, 4) > 0)
        s = R.Shape(int(rng.integers(1, 34)), int(rng.integers(0, 5)), int(rng.choice([16, 32, 48, 64, 96, 128, 256])), int(rng.integers(1, 5)),
                    R.ACTS[int(rng.integers(0, 2))], coords, embed, colors, bool(rng.integers(0, 2)),
                    H=int(rng.integers(1, 301)), W=int(rng.integers(1, 301)), msb_max=int(rng.choice([0, 1, 255, 2047, 2048, 65535])))
        if it % 8 == 0:      # the shapes of the codec's own defaults, where most draws would not land
            s = R.Shape(int(rng.choice([2, 4, 8])), int(rng.integers(1, 4)), s.bc, int(rng.integers(1, 3)), s.act, H=s.H, W=s.W, msb_max=s.msb_max)
        for req in R.REQUESTS:
            want = R.resolve(s, req)
            path = int(rng.integers(0, 3))
            rc, out = library_answer(s, req, path)
            tag = (it, s, s.H, s.W, s.msb_max, R.MODE_NAMES[req])
            if want is None:
                assert rc == E_UNSUPPORTED, tag
                refused += 1
            else:
                assert rc == 0 and out == want.words(), (tag, out, want.words())
                seen.add(want.instance())
            if req != R.DECODE:
                may_be_null = want is not None and R.is_fast(want.mode) and path != L.PATH_GENERIC
                st = null_msb_status(s, req, path)
                if want is None and path == L.PATH_MFMA:
                    assert st == E_UNSUPPORTED, tag          # (refused as a shape before the msb rule is asked)
                else:
                    assert (st != E_ARG) == may_be_null, (tag, st, lib.lbdrn_last_error())
                null_ok += may_be_null
        assert library_workspace(s) == restated_workspace(s), (it, s)
    assert seen == set(R.built_instances()) and refused > 1000 and null_ok > 300, (len(seen), refused, null_ok)


def test_apply_instance_refuses_what_the_entry_points_refuse():
    L, lib = _lib()
    s = R.Shape(4, 2, 64, 2)
    g, net = _structs(s)
    out = (ctypes.c_int32 * 8)()
    call = lambda word, o=out: lib.lbdrn_apply_instance(ctypes.byref(g), ctypes.byref(net), word, o)
    assert call(L.PATH_MFMA) == 0 and call(L.PATH_AUTO | L.EVAL_BACKGROUND) == 0 and list(out) == R.resolve(s, R.EVAL).words()
    assert call(3) == E_ARG and call(L.APPLY_DECODE | L.EVAL_FAST) == E_ARG and call(0, None) == E_ARG
    assert call(L.EVAL_X16) == 0 and list(out) == R.resolve(s, R.EVAL).words()      # (X16 without FAST is no flag, as in lbdrn_eval_sse)
    net.F += 1
    assert call(0) == E_ARG
    net.F -= 1
    net.bc = 96
    assert call(0) == E_UNSUPPORTED and b"bc=96" in lib.lbdrn_last_error()
    assert lib.lbdrn_abi_version() == 2


# ---------------------------------------------------------------------------------------------------------------------
# the float64 evaluation: what a sum can and cannot hide

def test_no_sum_of_the_census_can_hide_a_wrong_tile_or_two_exchanged_channels():
    """For every evaluation row (the decode rows are compared pixel by pixel and have no sum), from the float64 evaluation alone:
    replacing the predictions of ANY one tile of the row's plan by 0.5, or exchanging the predictions of ANY two adjacent
    channels, moves the SSE by more than ten times the relative bound the GPU test holds that row to (bound_of: 1e-11 for a
    canonical instance, 1e-6 for a fast or exact-operand one).  Also on the rasters with one more tile than compute units."""
    import oracle as O
    worst = {}
    for r in R.census() + R.big_rows():
        bound = R.bound_of(r)
        if bound is None:
            continue
        ref = R.reference(r)
        assert ref["sse64"] > 0 and ref["mx"] <= R.X16_MAX_MSB
        tile, chan = R.sensitivity(r, ref)
        assert tile > 10 * bound, (r.id, tile)
        assert chan is None or chan > 10 * bound, (r.id, chan)
        assert (chan is None) == (r.shape.C == 1)
        w = worst.setdefault(bound, [1.0, 1.0])
        worst[bound] = [min(w[0], tile), min(w[1], chan if chan is not None else 1.0)]
    assert set(worst) == {1e-11, 1e-6}
    for bound, (tile, chan) in sorted(worst.items()):
        print(f"bound {bound:g}: smallest relative move of the SSE by one tile at 0.5: {tile:.3e}, by two adjacent channels exchanged: {chan:.3e}")


def test_the_float64_evaluation_is_the_oracles_operation():
    """The float64 forward on the oracle's features against the oracle's own canonical float32 pass (what the canonical kernels
    compute bit for bit): the same operation, so the sums agree to float32 rounding -- held here to the 1e-6 the header gives a
    fast pass against the canonical one, and printed: it is the canonical pass's own distance from float64."""
    import oracle as O
    worst = 0.0
    for r in R.census() + R.big_rows():
        if r.request == R.DECODE:
            continue
        ref, s = R.reference(r), r.shape
        with O.hidden_activation(s.act):
            o = O.eval_sse(ref["msb"], ref["lab"], s.D, R.ocfg(s), ref["params"], s.bc, s.nl, ref["mx"])
        rel = abs(o - ref["sse64"]) / ref["sse64"]
        worst = max(worst, rel)
        assert rel <= 1e-6, (r.id, o, ref["sse64"])
    print(f"worst |canonical float32 - float64| / float64 over the evaluation rows: {worst:.3e}")
