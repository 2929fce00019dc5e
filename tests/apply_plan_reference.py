"""The planner of the fused apply pass restated (csrc/apply_mfma.hip: make_plan, serving_mode, resolve_apply, resolve_wapply,
the workspace sizing; csrc/apply_wide.inc: make_wapply_plan), and the census built on it: one row for each of the 32 kernel
instances of APPLY_INSTANCES / WAPPLY_INSTANCES at the smallest real shape that selects it, one row for each plan decision a
shape can flip, and one raster with more tiles than the device has compute units per kernel family and mode.  DESIGN.md 13.1.

Restated from the text of the sources, never from what the library answers: tests/test_apply_plan_host.py holds the constants and
lists to the source text, the answers to the library (lbdrn_apply_instance, lbdrn_apply_workspace, the NULL-msb rule of
lbdrn_eval_sse) and the census to the lists; tests/test_gpu_apply_instances.py runs the rows on the device.

A REAL shape, for the census: 2 to 32 bands (so that every row has adjacent channels to exchange), a window of D = 1..3, P = 0, 1 or
1 + 2 N_FREQ = 25 positional features per axis, relative or absolute colours, bc = 32, 64, 128 or 256, one or two hidden layers,
Sine or ReLU.  The smallest: fewest parameters, then fewest bands, then the reference's own switches first.  D = 0, one band,
colours off and the like appear as variant rows, by name.

A plain module: no fixture, no marker, no device."""
import functools
import itertools
import os
import re
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
APPLY_SOURCE, WIDE_SOURCE = os.path.join(CSRC, "apply_mfma.hip"), os.path.join(CSRC, "apply_wide.inc")

# ---------------------------------------------------------------------------------------------------------------------
# constants and lists, as the sources state them (source_constants() reads them back out of the text)

DECODE, EVAL, FAST, X16 = 0, 1, 2, 3
MODE_NAMES = ("DECODE", "EVAL", "EVAL_FAST", "EVAL_X16")
REQUESTS = (DECODE, EVAL, FAST, X16)
ACTS = ("sine", "relu")
APPLY_ROWS = ((1, DECODE), (2, DECODE), (4, DECODE), (1, EVAL), (2, EVAL), (4, EVAL), (1, FAST), (2, FAST), (1, X16), (2, X16))
WAPPLY_ROWS = ((8, 1), (8, 2), (16, 1), (16, 2))
WIDE_MODES = (DECODE, EVAL, FAST)
TILE_W, APPLY_THREADS, WA_THREADS, X16_PIECES, MFMA_PARTIALS = 64, 8 * 64, 256, 3, 1024
LDS_RESIDENT, LDS_WIDE = 160 * 1024, 64 * 1024
FAST_MAX_BANDS = 8            # resolve_apply: `mode_fast(mode) && net.C > 8` -- the 4x4-block last layer finishes channels 0..7
X16_MAX_MSB = 2047            # make_plan: MSB values that fp16 holds exactly
N_FREQ = 12
K = 5                         # the census images: 16-bit noise, MSB values 0..2047
CUS = 256                     # compute units of an MI355X: what the more-tiles rasters are sized for on the CPU (the GPU test asks the device)


def is_fast(mode):
    return mode in (FAST, X16)


def built_instances():
    """the 32: ("mfma", NT, mode, act) and ("wide", NT, NL, mode)"""
    return tuple(("mfma", nt, m, a) for nt, m in APPLY_ROWS for a in ACTS) + \
           tuple(("wide", nt, nl, m) for nt, nl in WAPPLY_ROWS for m in WIDE_MODES)


def source_constants():
    """What csrc/apply_mfma.hip and csrc/apply_wide.inc say, as text: the two lists, the mode numbers, the constants of the LDS maps."""
    with open(APPLY_SOURCE) as f:
        a = f.read()
    with open(WIDE_SOURCE) as f:
        w = f.read()
    modes = {name: int(v) for name, v in re.findall(r"\b(MODE_[A-Z0-9_]+) = (\d+)", a)}
    num = lambda text, pat: int(eval(re.search(pat, text).group(1), {}))   # (products of integer literals: "8 * 64")
    return {
        "modes": modes,
        "APPLY_ROWS": tuple((int(nt), modes[m]) for nt, m in re.findall(r"\bX\((\d+), (MODE_[A-Z0-9_]+)\)", a)),
        "WAPPLY_ROWS": tuple((int(nt), int(nl)) for nt, nl in re.findall(r"\bX\((\d+), (\d+)\)", a)),
        "WIDE_MODES": tuple(modes[m] for m in re.findall(r"LAUNCH\(nt, n, (MODE_[A-Z0-9_]+)\)", a)),
        "TILE_W": num(a, r"constexpr int TILE_W = ([\d* ]+);"),
        "APPLY_THREADS": num(a, r"constexpr int APPLY_WAVES = ([\d* ]+);") * 64,
        "WA_THREADS": num(w, r"constexpr int WA_THREADS = ([\d* ]+);"),
        "X16_PIECES": num(a, r"constexpr int X16_PIECES = ([\d* ]+);"),
        "MFMA_PARTIALS": num(a, r"constexpr int MFMA_PARTIALS = ([\d* ]+);"),
        "LDS_RESIDENT": num(a, r"if \(\(size_t\)q\.lds_floats \* 4 <= ([\d* ]+)\) break;"),
        "LDS_WIDE": num(w, r"if \(\(size_t\)q\.lds_floats \* 4 <= ([\d* ]+)\) break;"),
    }


# ---------------------------------------------------------------------------------------------------------------------
# a shape: what the planners read of lbdrn_geom and lbdrn_net

class Shape:
    def __init__(self, C, D, bc, nl, act="sine", coords=False, embed=False, colors=True, relative=True, H=17, W=65, msb_max=2047):
        self.C, self.D, self.bc, self.nl, self.act = C, D, bc, nl, act
        self.coords, self.embed, self.colors, self.relative = bool(coords), bool(embed and coords), bool(colors), bool(relative)
        self.P = 0 if not self.coords else (1 + 2 * N_FREQ if self.embed else 1)
        self.side = 2 * D + 1
        self.F = 2 * self.P + (C * self.side ** 2 if self.colors else 0)
        self.H, self.W, self.msb_max = H, W, msb_max

    def key(self):
        return (self.C, self.D, self.bc, self.nl, self.act, self.coords, self.embed, self.colors, self.relative, self.H, self.W, self.msb_max)

    def on(self, H, W):
        s = Shape(*self.key()[:9])
        s.H, s.W, s.msb_max = H, W, self.msb_max
        return s

    def params(self):
        return self.bc * self.F + self.bc + (self.nl - 1) * (self.bc * self.bc + self.bc) + self.C * self.bc + self.C

    def switches(self):
        return ("rel" if self.relative else "abs") + ("" if self.colors else "-nocolour") + ("-embed" if self.embed else "-coords" if self.coords else "")

    def __repr__(self):
        return f"C{self.C}-D{self.D}-bc{self.bc}-nl{self.nl}-{self.act}-{self.switches()}"


# ---------------------------------------------------------------------------------------------------------------------
# the planners

def serving_mode(mode, nt, x16):
    """the mode of the instance that serves a requested mode on nt tiles"""
    mfma_has = lambda m: (nt, m) in APPLY_ROWS
    if mode == X16 and not (x16 and mfma_has(X16)):
        mode = FAST
    if mode == FAST and not (mfma_has(FAST) or any(nt == w for w, _ in WAPPLY_ROWS)):
        mode = EVAL
    return mode


def make_plan(s, fast=False, x16=False):
    """k_apply_mfma: the weights resident in LDS beside one staged tile -> dict or None"""
    if s.act not in ACTS or s.bc % 32 or not any(nt == s.bc // 32 for nt, _ in APPLY_ROWS):
        return None
    if s.C > 32 or s.nl < 1 or s.nl > 15:
        return None
    NT, P, C, D = s.bc // 32, s.P, s.C, s.D
    ncolor = s.F - 2 * P
    S0 = P + ((ncolor + 1) // 2 + 3) // 4 * 4
    pair = bool(fast and NT <= 2 and s.colors and 1 <= D <= 3 and C % 2 == 0 and ncolor == C * s.side * s.side)
    RS = s.side * s.side - (1 if s.relative and D > 0 else 0)
    if pair:
        S0 = P + (C // 2) * RS
    x = bool(x16 and pair and s.relative and P == 0 and 1 <= max(s.msb_max, 1) <= X16_MAX_MSB and RS % 8 == 0)
    M16, half = RS // 8, s.bc // 2
    o = (C // 2) * M16 * X16_PIECES * 64 * NT * 4 if x else S0 * 64 * NT
    o += (s.nl - 1) * half * 64 * NT + half * 64 + s.nl * NT * 32 + 32 + 4
    pack = o
    o += 2 * 2 * (S0 - P) + 2
    fixed, SW = o, TILE_W + 2 * D
    for th in (16, 8, 4, 2, 1):
        rowt = fixed
        o = fixed + th * P + TILE_W * P + (C * (th + 2 * D) * SW if s.colors else 0)
        lds = max(o, rowt + 2 * APPLY_THREADS + 4)
        if lds * 4 <= LDS_RESIDENT:
            break
    else:
        return None
    return dict(NT=NT, S0=S0, TH=th, pair=int(pair), RS=RS, x16=int(x), M16=M16, pack=pack, lds=lds, ncolor=ncolor,
                pad_steps=S0 - P - ((ncolor + 1) // 2 if not pair else (C // 2) * RS),
                tiles_x=(s.W + TILE_W - 1) // TILE_W, tiles_y=(s.H + th - 1) // th)


def make_wapply_plan(s, fast=False):
    """k_apply_wide: the weights streamed, the Sine network -> dict or None"""
    if s.act != "sine" or s.bc % 16 or not any(nt == s.bc // 16 for nt, _ in WAPPLY_ROWS):
        return None
    if s.C > 16 or s.nl < 1 or s.nl > 2 or s.F < 1:
        return None
    NT, P, C, D = s.bc // 16, s.P, s.C, s.D
    ncolor = s.F - 2 * P
    S2 = s.side * s.side
    skip = bool(fast and s.colors and s.relative and D > 0 and ncolor == C * S2)
    Fe = s.F - C if skip else s.F
    G0 = ((Fe + 15) // 16 + 1) & ~1
    if ncolor < 1:
        return None
    pack = NT * G0 * 256 + (s.nl - 1) * NT * NT * 256 + NT * 256 + s.nl * NT * 16 + 16
    fixed, SW = 2 * max(ncolor, 1) + 2, TILE_W + 2 * D
    for th in (16, 8, 4, 2, 1):
        rowt = fixed
        o = (fixed + th * P + TILE_W * P + 3) & ~3
        o += C * (th + 2 * D) * SW if s.colors else 0
        lds = max(o, rowt + 2 * WA_THREADS + 4)
        if lds * 4 <= LDS_WIDE:
            break
    else:
        return None
    return dict(NT=NT, G0=G0, TH=th, skip=int(skip), Fe=Fe, pack=pack, lds=lds, pad_group=int(G0 != (Fe + 15) // 16),
                tiles_x=(s.W + TILE_W - 1) // TILE_W, tiles_y=(s.H + th - 1) // th)


def supported(s):
    """mfma_apply_supported: where LBDRN_PATH_MFMA does not answer LBDRN_E_UNSUPPORTED"""
    return make_plan(s) is not None or make_wapply_plan(s) is not None


class Answer:
    """What serves a request: family "mfma" / "wide", NT, NL (wide) or RELU (mfma), the serving mode, and the plan."""

    def __init__(self, family, plan, nl_or_relu, mode):
        self.family, self.plan, self.mode = family, plan, mode
        self.NT, self.TH = plan["NT"], plan["TH"]
        self.nl_or_relu = nl_or_relu
        self.pair, self.x16, self.M16, self.S0 = (plan["pair"], plan["x16"], plan["M16"], plan["S0"]) if family == "mfma" else (0, 0, 0, 0)
        self.skip, self.G0 = (plan["skip"], plan["G0"]) if family == "wide" else (0, 0)
        self.tiles_x, self.tiles_y = plan["tiles_x"], plan["tiles_y"]
        self.tiles = self.tiles_x * self.tiles_y

    def instance(self):
        if self.family == "mfma":
            return ("mfma", self.NT, self.mode, ACTS[self.nl_or_relu])
        return ("wide", self.NT, self.nl_or_relu, self.mode)

    def words(self):
        """lbdrn_apply_instance's out[8]"""
        return [1 if self.family == "mfma" else 2, self.NT, self.nl_or_relu, self.mode, self.TH,
                self.pair if self.family == "mfma" else self.skip, self.x16, self.tiles]


def resolve(s, request):
    """resolve_apply, then resolve_wapply where it says so: -> Answer, or None where the fused pass has no instance"""
    if not supported(s):
        return None
    mode = request
    if mode == X16:        # a hint: the fast plan where the x16 plan does not exist or has a shorter tile
        fp = make_plan(s, True, False)
        if fp is not None:
            xp = make_plan(s, True, True)
            if xp is None or xp["TH"] < fp["TH"]:
                mode = FAST
    requested = mode
    if is_fast(mode) and s.C > FAST_MAX_BANDS:
        mode = EVAL
    p = make_plan(s, is_fast(mode), mode == X16)
    if p is None:
        w = make_wapply_plan(s, is_fast(requested))
        if w is None:
            return None
        return Answer("wide", w, s.nl, serving_mode(requested, w["NT"], False))
    return Answer("mfma", p, ACTS.index(s.act), serving_mode(mode, p["NT"], bool(p["x16"])))


def instance_name(inst):
    if inst[0] == "mfma":
        return f"k_apply_mfma<{inst[1]}, {MODE_NAMES[inst[2]]}, {inst[3]}>"
    return f"k_apply_wide<{inst[1]}, {inst[2]}, {MODE_NAMES[inst[3]]}>"


def _up(n, a=256):
    return (n + a - 1) // a * a


def fused_workspace(s):
    """mfma_apply_workspace: the packed weights of the largest of a shape's plans, the SSE partials, one float (x16); 0: no plan"""
    p = make_plan(s)
    if p is None:
        w = make_wapply_plan(s)
        return 0 if w is None else _up(w["pack"] * 4) + _up(MFMA_PARTIALS * 8)
    s1 = s.on(s.H, s.W)
    s1.msb_max = 1
    q = make_plan(s1, True, True)
    return _up(max(p["pack"], q["pack"] if q is not None and q["x16"] else 0) * 4) + _up(MFMA_PARTIALS * 8) + 256


def generic_workspace(s, forward_workspace):
    """generic_apply_workspace (csrc/generic.hip); forward_workspace(chunk) is lbdrn_forward_workspace, another entry point's"""
    chunk = min(65536, s.H * s.W)
    return _up(chunk * s.F * 4) + _up(chunk * s.C * 4) + forward_workspace(chunk) + _up(256 * 8)


def apply_workspace(s, forward_workspace):
    """lbdrn_apply_workspace"""
    return max(generic_workspace(s, forward_workspace), fused_workspace(s))


# ---------------------------------------------------------------------------------------------------------------------
# the census

RASTERS = ((17, 65), (5, 33), (64, 64))   # tests/test_gpu_apply_blocks4.py: ragged both ways / fewer rows than a tile / four full tiles


class Row:
    """One case: a shape on a raster, a request, the instance and plan that serve it, and why the row is in the table."""

    def __init__(self, why, shape, request, note=""):
        self.why, self.shape, self.request, self.note = why, shape, request, note
        self.answer = resolve(shape, request)
        self.inst = self.answer.instance()
        self.id = f"{why}:{MODE_NAMES[request]}:{shape!r}:{shape.H}x{shape.W}"
        self.seed = zlib.crc32(self.id.encode()) & 0x7FFFFFFF

    def __repr__(self):
        return self.id


def real_shapes():
    """every real shape (module docstring), smallest first"""
    out = []
    for C, D, bc, nl, act in itertools.product(range(2, 33), (1, 2, 3), (32, 64, 128, 256), (1, 2), ACTS):
        for k, (coords, embed) in enumerate(((False, False), (True, False), (True, True))):
            for relative in (True, False):
                s = Shape(C, D, bc, nl, act, coords, embed, True, relative)
                out.append(((s.params(), C, k, not relative, D), s))
    out.sort(key=lambda t: t[0])
    return [s for _, s in out]


@functools.lru_cache(maxsize=None)
def _resolved(request):
    return tuple((s, a) for s in real_shapes() if (a := resolve(s, request)) is not None)


def _d4_shapes():
    """D = 4, which no real shape has: where a tile height needs it"""
    return [Shape(C, 4, bc, nl) for bc, nl, C in itertools.product((128, 256), (1, 2), range(2, 17))]


def _first(pred, request, required=True, shapes=None):
    pool = _resolved(request) if shapes is None else [(s, a) for s in shapes if (a := resolve(s, request)) is not None]
    hit = next((s for s, a in pool if pred(s, a)), None)
    assert hit is not None or not required, "no real shape selects this"
    return hit


def _on_raster(rows):
    """the three rasters dealt over the rows in turn, so that each kernel family and mode meets all of them"""
    return [Row(why, s.on(*RASTERS[k % len(RASTERS)]), request, note) for k, (why, s, request, note) in enumerate(rows)]


def reachable_th():
    """{("mfma" | "wide", TH)}: the tile heights the two LDS budgets produce over C <= 32 (resident) and C <= 16 (streamed), D = 0..4,
    every switch, width, depth and activation.  What is missing from {16, 8, 4, 2, 1} cannot be planned: see UNREACHABLE_TH."""
    seen = set()
    for C, D, bc, nl in itertools.product(range(1, 33), range(0, 5), (32, 64, 128, 256), (1, 2)):
        for coords, embed in ((False, False), (True, False), (True, True)):
            s = Shape(C, D, bc, nl, "sine", coords, embed)
            for req in (EVAL, FAST):
                a = resolve(s, req)
                if a is not None:
                    seen.add((a.family, a.TH))
    return seen


# The resident kernel reaches every height: its 160 KB hold the weights too, and a tile of 16, 8, 4, 2 or 1 rows is what is left
# (TH = 4 and 2 with more than 8 bands only, so no fast instance runs them).  The streaming kernel's 64 KB = 16,384 floats hold
# the offset table and the window only: at D <= 3 the largest, 16 bands at D = 3, stages (TH + 6) x 70 floats a band beside 1,570
# of table -- 8 rows do not fit, 4 do.  TH = 2 takes D = 4, a window no real shape has: 16 bands, (TH + 8) x 72 a band beside
# 2,594 is 16,418 at 4 rows and 14,114 at 2 (15,764 with the embedding's tables).  So TH = 1 is never planned for k_apply_wide
# within 16 bands and D <= 4, and its one-row walk runs only behind k_apply_mfma's.
UNREACHABLE_TH = (("wide", 1),)


@functools.lru_cache(maxsize=None)
def census():
    """-> tuple of Rows: "instance" rows (the 32), then variant rows by name"""
    rows = []
    for inst in built_instances():
        req = inst[2] if inst[0] == "mfma" else inst[3]     # the request that asks for the instance's own mode
        rows.append(("instance", _first(lambda s, a: a.instance() == inst, req), req, instance_name(inst)))
    V = rows.append
    # every tile height either budget produces (the instance rows have 16); D = 4 for the streaming kernel's TH = 2
    for fam, th in sorted(reachable_th(), key=lambda t: (t[0], -t[1])):
        if th == 16:
            continue
        for req, tag in ((EVAL, ""), (FAST, "-fast")):
            hit = lambda s, a: a.family == fam and a.TH == th and a.mode == req
            s = _first(hit, req, required=False) or _first(hit, req, required=False, shapes=_d4_shapes())
            if s is not None:
                V((f"TH{th}-{fam}{tag}", s, req, "the tile halved until the LDS map fits"))
    # pair: on, and off by each of its three causes (a fast instance serves all four)
    V(("pair-on", _first(lambda s, a: a.family == "mfma" and a.pair and a.mode == FAST and s.C >= 4, FAST), FAST, "channel pairs"))
    V(("pair-off-odd-bands", _first(lambda s, a: a.family == "mfma" and a.mode == FAST and s.C % 2 == 1, FAST), FAST, "C odd"))
    V(("pair-off-D0", Shape(4, 0, 64, 2), FAST, "no window"))
    V(("pair-off-no-colours", Shape(4, 2, 32, 1, coords=True, embed=True, colors=False), FAST, "USE_COLORS off"))
    # skip in the wide fast pass
    V(("skip-on", _first(lambda s, a: a.family == "wide" and a.skip and a.NT == 16, FAST), FAST, "window centres left out"))
    V(("skip-off-absolute", _first(lambda s, a: a.family == "wide" and not a.skip and not s.relative, FAST), FAST, "absolute colours"))
    V(("skip-off-D0", Shape(4, 0, 256, 1), FAST, "no window"))
    # padding: an odd group count rounded up to even (wide), padding steps in S0 (resident)
    V(("pad-group", _first(lambda s, a: a.family == "wide" and a.plan["pad_group"], EVAL), EVAL, "G0 rounded up to even"))
    V(("no-pad-group", _first(lambda s, a: a.family == "wide" and not a.plan["pad_group"], EVAL), EVAL, "G0 even as it is"))
    V(("pad-steps", _first(lambda s, a: a.family == "mfma" and a.plan["pad_steps"] == 3, EVAL), EVAL, "three zero-weight steps in S0"))
    V(("no-pad-steps", _first(lambda s, a: a.family == "mfma" and a.plan["pad_steps"] == 0 and not s.coords, EVAL), EVAL, "S0 full"))
    # x16: MFMAs per channel pair and weight piece
    for m16 in (1, 3, 6):
        V((f"x16-M16-{m16}", _first(lambda s, a: a.mode == X16 and a.M16 == m16 and a.NT == 2, X16), X16, f"RS = {8 * m16}"))
    qualifies = lambda s, a: a.family == "mfma" and a.mode == FAST and a.pair and s.relative and s.P == 0   # .. but for the x16 pack's size
    V(("x16-to-fast-no-room", _first(lambda s, a: qualifies(s, a) and make_plan(s, True, True) is None, X16), X16,
       "the x16 pack does not fit beside a one-row tile"))
    V(("x16-to-fast-shorter-tile", _first(lambda s, a: qualifies(s, a) and make_plan(s, True, True) is not None, X16), X16,
       "the x16 pack leaves a shorter tile than the fast plan's"))
    V(("x16-to-fast-absolute", _first(lambda s, a: a.family == "mfma" and a.mode == FAST and not s.relative and a.pair, X16), X16, "absolute colours: no x16 plan"))
    V(("x16-to-fast-positional", _first(lambda s, a: a.family == "mfma" and a.mode == FAST and s.coords and a.pair, X16), X16, "P > 0: no x16 plan"))
    # more than 8 bands: the canonical instance serves a fast request
    V(("C9-fast-request", _first(lambda s, a: s.C == 9 and a.family == "mfma", FAST), FAST, "served by the canonical instance"))
    V(("C9-x16-request", _first(lambda s, a: s.C == 9 and a.family == "mfma" and a.NT == 2, X16), X16, "served by the canonical instance"))
    V(("bc128-fast-request", _first(lambda s, a: a.family == "mfma" and a.NT == 4, FAST), FAST, "NT 4 has no fast instance"))
    # P = 0, 1, 25 on either family
    for fam in ("mfma", "wide"):
        for P in (0, 1, 1 + 2 * N_FREQ):
            V((f"P{P}-{fam}", _first(lambda s, a: a.family == fam and s.P == P and s.nl == 2, DECODE), DECODE, "positional features per axis"))
            V((f"P{P}-{fam}-fast", _first(lambda s, a: a.family == fam and s.P == P and is_fast(a.mode), FAST), FAST, "the same in the fast pass"))
    V(("no-colours-coords-decode", Shape(3, 2, 64, 2, coords=True, embed=True, colors=False), DECODE, "USE_COLORS off: F = 2 P"))
    V(("no-colours-coords-eval", Shape(3, 2, 128, 1, "relu", coords=True, colors=False), EVAL, "USE_COLORS off, P = 1: F = 2"))
    # one band, both families
    V(("one-band-mfma", Shape(1, 2, 32, 2), FAST, "C = 1"))
    V(("one-band-wide", Shape(1, 2, 256, 2), FAST, "C = 1"))
    return tuple(_on_raster(rows))


def big_rows(cus=CUS):
    """One raster with one more tile than the device has compute units per kernel family and mode: 3 columns by 16 cus + 1 rows at
    TH = 16.  k_apply_mfma on 2 bands (the exact-operand pass wants an even count); k_apply_wide at bc = 256 on the fewest bands
    at which it plans TH = 16 -- which the restatement says is every count up to 13 at D = 1, so: 2, like the other family."""
    H, W = 16 * cus + 1, 3
    wide_C = next(C for C in range(2, 17) if make_wapply_plan(Shape(C, 1, 256, 1))["TH"] == 16)
    rows = []
    for req in REQUESTS:
        rows.append(Row("tiles>CUs", Shape(2, 1, 64, 2, H=H, W=W), req, "k_apply_mfma walks more than one tile"))
    for req in WIDE_MODES:
        rows.append(Row("tiles>CUs", Shape(wide_C, 1, 256, 1, H=H, W=W), req, "k_apply_wide walks more than one tile"))
    for r in rows:
        assert r.answer.TH == 16 and r.answer.tiles == cus + 1 and r.answer.mode == r.request, r.id
    return tuple(rows)


def table_text(rows=None):
    """the census as a markdown table"""
    rows = census() if rows is None else rows
    out = ["| row | request | shape | raster | instance | TH | tiles | pair / skip | x16 (M16) | S0 / G0 |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a = r.answer
        out.append(f"| {r.why} | {MODE_NAMES[r.request]} | {r.shape!r} F={r.shape.F} | {r.shape.H} x {r.shape.W} | `{instance_name(r.inst)}` | {a.TH} | "
                   f"{a.tiles_y} x {a.tiles_x} | {a.pair if a.family == 'mfma' else a.skip} | {a.x16} ({a.M16 if a.x16 else '-'}) | "
                   f"{a.S0 if a.family == 'mfma' else a.G0} |")
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the float64 evaluation of a row

def mixed_params(rng, F, bc, C, nl, act):
    """state_dict order, weights of mixed magnitude as in tests/test_gpu_apply_blocks4.py (_mixed_params): rows of every layer scaled by
    powers of two between 1/8 and 2, the last layer's between 1/16 and 4, a last bias of up to +-4 on every other channel (the
    rest near zero).  A ReLU net has no w0 = 30 in front of its activations: its hidden weights are 10 times larger."""
    gain = 10.0 if act == "relu" else 1.0
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = (2.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        w = rng.uniform(-b, b, (bc, nin)) * np.exp2(rng.integers(-3, 2, (bc, 1)))
        parts += [w.ravel(), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    w = rng.uniform(-b, b, (C, bc)) * np.exp2(rng.integers(-4, 3, (C, 1)))
    bias = np.where(np.arange(C) % 2 == 0, rng.choice([-1.0, 1.0], C) * rng.uniform(1.0, 4.0, C), rng.uniform(-1e-3, 1e-3, C))
    parts += [w.ravel(), bias]
    return np.concatenate(parts).astype(np.float32)


def ocfg(s):
    import oracle as O
    return O.FeatCfg(s.coords, s.embed, 1.4, N_FREQ, s.colors, s.relative)


def row_inputs(row):
    """-> (image [C,H,W] uint16 noise, parameters float32): the row's own seed"""
    s = row.shape
    rng = np.random.default_rng(row.seed)
    img = rng.integers(0, 1 << 16, (s.C, s.H, s.W)).astype(np.uint16)
    return img, mixed_params(rng, s.F, s.bc, s.C, s.nl, s.act)


_REF = {}


def reference(row):
    """The float64 evaluation of a row, computed once and left unchanged: the oracle's float32 features and labels, the float32
    parameters, everything after them in float64 (tests/train_step_f64.py) -> dict(img, params, msb, lab, mx, y64 [N, C], sse64)"""
    if row.id not in _REF:
        import oracle as O
        import train_step_f64 as T
        s = row.shape
        img, p = row_inputs(row)
        msb, lab, mx = O.split_bits(img, K)
        x = O.features(msb, s.D, ocfg(s), mx)
        _, _, y = T.forward_f64(p.astype(np.float64), x.astype(np.float64), s.F, s.bc, s.C, s.nl, s.act)
        d = y - lab.astype(np.float64)
        for a in (img, p, msb, lab, y):
            a.setflags(write=False)
        _REF[row.id] = dict(img=img, params=p, msb=msb, lab=lab, mx=mx, y64=y, sse64=float(np.sum(d * d)))
    return _REF[row.id]


def bound_of(row):
    """the relative bound the GPU test holds the row's sum to: the 1e-11 of tests/test_gpu_fuzz.py between the canonical sum and
    the oracle's / the generic path's, the header's 1e-6 for a fast or exact-operand instance; a decode row is compared bit for
    bit and has no sum"""
    return {DECODE: None, EVAL: 1e-11, FAST: 1e-6, X16: 1e-6}[row.answer.mode]


def sensitivity(row, ref=None):
    """From the float64 evaluation alone: the smallest relative move of the SSE over (a) every tile of the row's plan, its
    predictions replaced by 0.5, and (b) every pair of adjacent channels, their predictions exchanged -> (tile, channel); the
    channel figure is None for one band."""
    ref = reference(row) if ref is None else ref
    s, a = row.shape, row.answer
    y = ref["y64"].reshape(s.H, s.W, s.C)
    lab = ref["lab"].astype(np.float64).reshape(s.H, s.W, s.C)
    e = (y - lab) ** 2
    flat = (0.5 - lab) ** 2
    gain = (flat - e).sum(axis=2)                                  # per pixel: what replacing its predictions by 0.5 adds
    pad_h, pad_w = a.tiles_y * a.TH - s.H, a.tiles_x * TILE_W - s.W
    g = np.pad(gain, ((0, pad_h), (0, pad_w))).reshape(a.tiles_y, a.TH, a.tiles_x, TILE_W).sum(axis=(1, 3))
    tile = float(np.abs(g).min() / ref["sse64"])
    chan = None
    if s.C > 1:
        swapped = ((y[:, :, 1:] - lab[:, :, :-1]) ** 2 + (y[:, :, :-1] - lab[:, :, 1:]) ** 2 - e[:, :, 1:] - e[:, :, :-1]).sum(axis=(0, 1))
        chan = float(np.abs(swapped).min() / ref["sse64"])
    return tile, chan
