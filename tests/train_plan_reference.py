"""Which template instance of the fused bc = 64 training step runs a shape: a plain Python restatement of make_train_plan and
dispatch_train of csrc/train_mfma.hip (with stream_lds of csrc/train_stream.inc for the LDS bound), the three instance lists and
the constants of that source read out of its text, and the census of instances the GPU test tests/test_gpu_train_instances.py
steps one by one.

A plain module: no fixture, no marker, no device.  tests/test_train_plan_host.py holds it to the source text and, where the
library tells (lbdrn_train_step_features, lbdrn_train_group_size), to the library.

An instance is (kernel, LQ, NL, NT0C, ACT): kernel "stream" (k_train_stream<LQ, NL, PD, NT0C, ACT>), "split"
(k_train_split<LQ, NT0C, ACT>, NL = 2) or "tile" (k_train_mfma<LQ, NL>, Sine, NT0C = 0); NT0C = 0 is the generic weight-gradient
loop.  "generic": the shape has no fused bc = 64 step."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
TRAIN_SOURCE = os.path.join(CSRC, "train_mfma.hip")

# ---------------------------------------------------------------------------------------------------------------------
# the intended values (tests/test_train_plan_host.py asserts that the source states the same)

STREAM = ((16, 1, 0), (16, 2, 0), (24, 1, 0), (24, 2, 0), (24, 2, 6), (32, 1, 0), (32, 2, 0), (48, 1, 0), (48, 2, 0), (48, 2, 12),
          (52, 1, 0), (52, 2, 13), (64, 1, 0), (64, 2, 0), (64, 2, 16))   # (LQ, NL, NT0C) of k_train_stream, ascending LQ
SPLIT = ((24, 6), (48, 12), (64, 16), (96, 24))                 # (LQ, NT0C) of k_train_split
TILE = ((16, 3), (32, 3), (52, 3))                              # (LQ, NL) of the tile kernel
STREAM_LQ = tuple(sorted({lq for lq, nl, c in STREAM}))         # layer-0 quarter lengths of the streamed step
TILE_LQ = tuple(lq for lq, nl in TILE)                          # ... of the nl = 3 tile kernel
STRAIGHT = tuple((lq, c) for lq, nl, c in STREAM if c)          # (LQ, NT0) with a straight-line weight-gradient schedule
SPLIT_WIDE_LQ = 96                          # 256 < Fe <= 384 at nl = 2: k_train_split only
MAX_GROUP = 4                               # fits per launch (blockIdx.y)
LDS_BOUND = 160 * 1024                      # bytes of LDS a workgroup may ask for
MAX_C, BC = 16, 64
ACTS = ("sine", "relu")

GENERIC = "generic"


def source_constants(text=None):
    """The same lists and constants as csrc/train_mfma.hip states them."""
    if text is None:
        with open(TRAIN_SOURCE) as f:
            text = f.read()
    k = {}
    for name in ("STREAM", "SPLIT", "TILE"):                # one X-macro list each: #define NAME_INSTANCES(X) X(..) X(..) ..
        body, = re.findall(r"#define %s_INSTANCES\(X\)((?:[ \\\n]*X\([\d, ]+\))+)\n" % name, text)
        k[name] = tuple(tuple(int(x) for x in row.split(",")) for row in re.findall(r"\(([\d, ]+)\)", body))
    for name in ("SPLIT_WIDE_LQ", "MAX_GROUP"):
        found = re.findall(r"constexpr int %s = (\d+);" % name, text)
        assert len(found) == 1, (name, found)
        k[name] = int(found[0])
    bounds = re.findall(r"\* 4 [<>]=? (\d+) \* 1024", text)      # the static_assert over the streamed list and the tile kernel's check
    assert len(bounds) == 2 and len(set(bounds)) == 1, bounds
    k["LDS_BOUND"] = int(bounds[0]) * 1024
    # how the lists are read: the schedule of exactly NT0 strips where there is one, k_train_split by (LQ, NT0), the B >= 2 rule
    assert "if (lq == LQ && nl == NL && nt0 == NT0C) return NT0C;" in text
    assert "p.wave == STEP_STREAM && net.nl == 2 && split_nt0c(p.LQ) == p.NT0" in text
    assert "split && (B >= 2 || split_only(A.p))" in text
    assert "(alone && count == 1 && split_available(A.p, net)) || split_only(A.p)" in text
    return k


# ---------------------------------------------------------------------------------------------------------------------
# the LDS maps (csrc/train_stream.inc: stream_lds; csrc/train_mfma.hip: the tile kernel's lds_floats)

def stream_lds_floats(LQ, NL):
    SGP, SHP, SOP, WB, WPT = 260, 68, 20, 64, 68
    SHSZ, SZOSZ, SZTSZ, SRED = WB * SHP + 48, WB * SOP + 48, 64 * WPT, 8 + 2 * 64
    G0 = LQ // 4
    NST = (G0 + 2) // 2
    n = (G0 + 1) * SGP
    wpx = n + ((16 - n % 32) + 32) % 32
    stage = 4 * wpx
    stage_end = stage + 4 * G0 * 256
    alias = 2 * (NST - 1) - 1 >= (SHSZ + SRED + 1023) // 1024 - 1
    r = stage + ((SHSZ + SRED + 3) & ~3) if alias else stage
    r += (NL - 1) * SHSZ + SZOSZ + NL * SZTSZ
    small = (NL - 1) * 16 * 256
    total = max(r, stage_end)
    if NL > 1:
        wht = max(r, stage_end + small)
        if (wht + small + (0 if alias else SHSZ + SRED)) * 4 <= LDS_BOUND:
            total = wht + small
    if not alias:
        total += SHSZ + SRED
    return total + 256


def tile_lds_floats(LQ, NT0, nl):
    TB, TBC, HP, TP, OP = 32, 64, 68, 36, 20
    return TB * (4 * LQ + 4) + 16 * NT0 * TP + 2 * nl * TB * HP + 2 * nl * TBC * TP + TB * OP + 16 * TP + TB + 16


# ---------------------------------------------------------------------------------------------------------------------
# the plan and the dispatch

def centre_skipping_fe(use_colors, relative, P, C, D, F):
    """Features the streamed step multiplies (centre_skipping_map): F - C where the window centres are exact zeros."""
    side = 2 * D + 1
    if use_colors and relative and D > 0 and F == 2 * P + C * side * side:
        return F - C
    return F


def plan(use_colors, relative, P, C, D, F, nl, act):
    """make_train_plan at bc = 64 -> None (no fused step) or dict(kind "stream" / "tile", LQ, Fe, NT0)."""
    if act not in ACTS or nl < 1 or nl > 3 or C > MAX_C or F < 1:
        return None
    if act == "relu" and nl > 2:
        return None
    if nl <= 2:   # the streamed step or k_train_split, or nothing
        Fe = centre_skipping_fe(use_colors, relative, P, C, D, F)
        LQ = next((lq for lq, n, c in STREAM if n == nl and Fe <= 4 * lq), 0)
        if not LQ and nl == 2 and Fe <= 4 * SPLIT_WIDE_LQ:
            LQ = SPLIT_WIDE_LQ
        if not LQ:
            return None
        return dict(kind="stream", LQ=LQ, Fe=Fe, NT0=dict(SPLIT)[LQ] if LQ == SPLIT_WIDE_LQ else (Fe + 15) // 16)
    RP = (F + C + 3) // 4 * 4
    LQ = next((lq for lq, n in TILE if n == nl and F <= 4 * lq and RP <= 4 * lq + 4), 0)
    NT0 = (F + 15) // 16
    if not LQ or tile_lds_floats(LQ, NT0, nl) * 4 > LDS_BOUND:
        return None
    return dict(kind="tile", LQ=LQ, Fe=F, NT0=NT0)


def takes_groups(p):
    return p is not None and p["kind"] == "stream"


def split_available(p, nl):
    return p["kind"] == "stream" and nl == 2 and (p["LQ"], p["NT0"]) in SPLIT


def instance(use_colors, relative, P, C, D, F, nl, act, alone=False, count=1, B=2):
    """The kernel that steps a minibatch of B rows of `count` fits of this shape (lbdrn_train_epoch[_group], PATH_MFMA)."""
    p = plan(use_colors, relative, P, C, D, F, nl, act)
    if p is None:
        return GENERIC
    assert 1 <= count <= MAX_GROUP and (count == 1 or takes_groups(p)) and B >= 1
    if p["kind"] == "tile":
        inst = ("tile", p["LQ"], nl, 0, "sine")
    else:
        split_only = p["LQ"] == SPLIT_WIDE_LQ
        split = (alone and count == 1 and split_available(p, nl)) or split_only
        if split and (B >= 2 or split_only):
            inst = ("split", p["LQ"], 2, p["NT0"], act)
        else:
            inst = ("stream", p["LQ"], nl, p["NT0"] if (p["LQ"], nl, p["NT0"]) in STREAM else 0, act)
    assert inst in built_instances(), inst      # dispatch_train refuses what no list names: a plan never gets there
    return inst


@functools.lru_cache(maxsize=None)
def built_instances():
    """Every instance the three lists name (what the library is compiled with): the loops, the straight-line schedules and
    k_train_split per activation, then the tile kernel's."""
    out = []
    for act in ACTS:
        out += [("stream", lq, nl, c, act) for lq, nl, c in sorted(STREAM, key=lambda r: r[2] > 0)]
        out += [("split", lq, 2, c, act) for lq, c in SPLIT]
    return tuple(out + [("tile", lq, nl, 0, "sine") for lq, nl in TILE])


def instance_id(inst, Fe):
    kernel, lq, nl, nt0c, act = inst
    if kernel == "split":
        return f"split-LQ{lq}-nt{nt0c}-{act}-Fe{Fe}"
    if kernel == "tile":
        return f"tile-LQ{lq}-nl{nl}-{act}-Fe{Fe}"
    return f"stream-LQ{lq}-nl{nl}-{'loop' if nt0c == 0 else 'straight%d' % nt0c}-{act}-Fe{Fe}"


# ---------------------------------------------------------------------------------------------------------------------
# real shapes: the switches of FeatCfg (coordinates, embedding, colours, relative; n_freq = 12 as constants.py has it),
# C <= 16 bands, D <= 3

class Shape:
    """One feature configuration + network: what a census row steps."""

    def __init__(self, coords, embed, colors, relative, C, D, nl, act):
        self.coords, self.embed, self.colors, self.relative = bool(coords), bool(embed), bool(colors), bool(relative)
        self.C, self.D, self.nl, self.act = C, D, nl, act
        self.P = 0 if not coords else (25 if embed else 1)
        side = 2 * D + 1
        self.F = 2 * self.P + (C * side * side if colors else 0)
        self.Fe = centre_skipping_fe(self.colors, self.relative, self.P, C, D, self.F)

    def key(self):
        return (self.colors, self.relative, self.P, self.C, self.D, self.F, self.nl, self.act)

    def plan(self):
        return plan(*self.key())

    def instance(self, alone=False, count=1, B=2):
        return instance(*self.key(), alone=alone, count=count, B=B)

    def featcfg(self):
        from lbdrn_hip.features import FeatCfg
        return FeatCfg(self.coords, self.embed, 1.4, 12, self.colors, self.relative, self.act)

    def size(self):
        """what "smallest" means: fewest features multiplied, then fewest parameters, bands, window, table columns"""
        return (self.Fe, self.F, self.C, self.D, self.P, self.relative)

    def __repr__(self):
        sw = "".join(c if on else "-" for c, on in zip("cekr", (self.coords, self.embed, self.colors, self.relative)))
        return f"C{self.C} D{self.D} {sw} F{self.F} nl{self.nl} {self.act}"


@functools.lru_cache(maxsize=None)
def feature_configs():
    """Every (coords, embed, colors, relative, C, D) with F >= 1, one per distinct (F, Fe, C) -- the smallest first."""
    seen, out = set(), []
    cands = []
    for coords, embed in ((0, 0), (1, 0), (1, 1)):
        for colors in (1, 0):
            for relative in (1, 0):
                for D in range(4):
                    for C in range(1, MAX_C + 1):
                        s = Shape(coords, embed, colors, relative, C, D, 2, "sine")
                        if s.F >= 1 and (colors or (relative and D == 0)):   # (without colours D and RELATIVE change nothing: one form)
                            cands.append(s)
    for s in sorted(cands, key=Shape.size):
        k = (s.F, s.Fe, s.C, s.colors, s.relative and s.D > 0)
        if k not in seen:
            seen.add(k)
            out.append((s.coords, s.embed, s.colors, s.relative, s.C, s.D))
    return tuple(out)


def shapes(nl, act):
    return [Shape(*c, nl, act) for c in feature_configs()]


@functools.lru_cache(maxsize=None)
def reachable_fe(nl=2):
    """Sorted Fe of every real shape whose step at this nl is a streamed one (the class boundaries are about those)."""
    return tuple(sorted({s.Fe for s in shapes(nl, "sine") if takes_groups(s.plan())}))


BOUNDARIES = ((64, 65), (96, 97), (128, 129), (192, 193), (208, 209))   # Fe classes of the streamed step: LQ 16|24|32|48|52|64


def nearest(side, edge):
    """The reachable Fe nearest to a class edge: the largest <= edge ("lo") or the smallest >= edge ("hi")."""
    fe = reachable_fe(2)
    return max(f for f in fe if f <= edge) if side == "lo" else min(f for f in fe if f >= edge)


class Row:
    """One census row: the shape, whether the fit says it is alone, the instance that steps its minibatches of two rows
    or more, and why the row is in the table."""

    def __init__(self, shape, alone, why):
        self.shape, self.alone, self.why = shape, alone, why
        self.inst = shape.instance(alone=alone, count=1, B=2)
        p = shape.plan()
        self.Fe, self.NT0, self.LQ = p["Fe"], p["NT0"], p["LQ"]
        self.id = instance_id(self.inst, self.Fe)

    @property
    def family(self):
        k, lq, nl, nt0c, act = self.inst
        if k == "stream":
            return "stream-loop" if nt0c == 0 else "stream-straight"
        if k == "split":
            return "split-wide" if lq == SPLIT_WIDE_LQ else "split"
        return "tile"


def _smallest(inst):
    kernel, lq, nl, nt0c, act = inst
    for s in shapes(nl, act):
        for alone in (False, True):
            if s.instance(alone=alone, count=1, B=2) == inst:
                return Row(s, alone, "instance")
    return None


@functools.lru_cache(maxsize=None)
def census():
    """-> (rows, unreachable): rows = one Row per built instance (its smallest real shape) followed by the rows that the class
    boundaries and the multiple-of-16 rule add; unreachable = the built instances no real shape selects (there are none)."""
    rows, unreachable, seen = [], [], set()
    for inst in built_instances():
        r = _smallest(inst)
        if r is None:
            unreachable.append(inst)
        else:
            rows.append(r)
            seen.add((r.shape.key(), r.alone))

    def add(fe, why):
        s = next(s for s in shapes(2, "sine") if s.Fe == fe and takes_groups(s.plan()))
        if (s.key(), False) not in seen:
            seen.add((s.key(), False))
            rows.append(Row(s, False, why))

    for lo, hi in BOUNDARIES:
        add(nearest("lo", lo), f"boundary {lo}|{hi}, below")
        add(nearest("hi", hi), f"boundary {lo}|{hi}, above")
    for lq in STREAM_LQ + (SPLIT_WIDE_LQ,):
        for full in (True, False):
            have = [r for r in rows if r.LQ == lq and r.inst[0] != "tile" and (r.Fe % 16 == 0) == full]
            if not have:
                fe = next((f for f in reachable_fe(2) if (f % 16 == 0) == full and
                           next(s for s in shapes(2, "sine") if s.Fe == f).plan()["LQ"] == lq), None)
                if fe is not None:
                    add(fe, f"LQ {lq}: a last strip that is {'full' if full else 'part-filled'}")
    return tuple(rows), tuple(unreachable)


def table_text():
    rows, _ = census()
    lines = ["| instance | smallest shape | F | Fe | NT0 | why |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| `{r.id}`{' (alone)' if r.alone else ''} | {r.shape!r} | {r.shape.F} | {r.Fe} | {r.NT0} | {r.why} |")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of a row (shared by the CPU check of the ReLU kink condition and the GPU test)

H, W, K = 13, 11, 5          # 143 pixels, H, W > D (the other half of the domain -- H <= D or W <= D, N < 64 -- is stepped by
                             # tests/test_gpu_thin_rasters.py on the rows of tests/thin_cases.py)
BS = 100                     # minibatches of 100 rows (two workgroups, the second part-filled) and of 43 (less than one)
BS_TAIL = 71                 # 71, 71, 1: a one-row tail
KINK = 1e-5                  # ReLU: no hidden pre-activation of the float64 reference within this of 0, relative to the layer's largest


def init_params(rng, F, C, nl, act):
    """uniform weights at the reference's scales (LBDRNmodel.py), the ReLU net's ten times larger (tests/test_gpu_fuzz.py:
    no w0 = 30 in front of a ReLU)"""
    gain = 10.0 if act == "relu" else 1.0
    parts = []
    for l in range(nl):
        nin = F if l == 0 else BC
        b = (1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, BC * nin), rng.uniform(-b, b, BC)]
    b = np.sqrt(6.0 / BC) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * BC), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


def fit_inputs(shape, seed, fit):
    """Image, initial parameters and permutation of fit `fit` of a row: all three differ between the fits, and so does
    the largest MSB value (fit k draws k + 9 bits)."""
    rng = np.random.default_rng([seed, fit, shape.F, shape.C, shape.nl])
    img = rng.integers(0, 1 << (9 + fit), (shape.C, H, W)).astype(np.uint16)
    img[0, 0, 0] |= np.uint16(1 << K)
    p0 = init_params(rng, shape.F, shape.C, shape.nl, shape.act)
    perm = rng.permutation(H * W).astype(np.int64)
    return img, p0, perm


def first_step_f64(shape, seed):
    """Fit 0's first minibatch in float64: -> (x, t, p0, batch, loss, gradient)"""
    import oracle as O
    import train_step_f64 as T
    img, p0, perm = fit_inputs(shape, seed, 0)
    msb, lab, mx = O.split_bits(img, K)
    ocfg = O.FeatCfg(shape.coords, shape.embed, 1.4, 12, shape.colors, shape.relative)
    x = O.features(msb, shape.D, ocfg, mx).astype(np.float64)
    t = lab.astype(np.float64)
    b = perm[:BS]
    loss, g = T.loss_and_grad_f64(p0.astype(np.float64), x[b], t[b], shape.F, BC, shape.C, shape.nl, shape.act)
    return x, t, p0, b, loss, g


@functools.lru_cache(maxsize=None)
def row_seed(row_id):
    """The seed of a row's inputs.  Sine: 0.  ReLU: the first seed at which the float64 reference of fit 0's first
    minibatch keeps every hidden pre-activation KINK away from 0 (a condition on the inputs: a float32 pre-activation
    may otherwise sit on the other side of the kink from the float64 one, which is no kernel error)."""
    import train_step_f64 as T
    row = next(r for r in census()[0] if r.id == row_id)
    if row.shape.act != "relu":
        return 0
    for seed in range(64):
        x, t, p0, b, _, _ = first_step_f64(row.shape, seed)
        if T.kink_margin(p0, x[b], row.shape.F, BC, row.shape.C, row.shape.nl) >= KINK:
            return seed
    raise AssertionError(f"no seed below 64 keeps {row_id} off the ReLU kink")
