"""Which template instance of the bc = 128 / 256 training step runs a shape: a plain Python restatement of make_wide_plan,
wide_ws_layout and the launch geometry of csrc/train_wide.inc (k_train_half<LQ, NL, NT> -> k_dw_wide<NT, NL> -> k_reduce_adam),
the constants and dispatch cases of that source read out of its text, and the census of instances the GPU test
tests/test_gpu_wide_train_instances.py steps one by one.

A plain module: no fixture, no marker, no device.  tests/test_wide_plan_host.py holds it to the source text and, where the
library tells without a device (lbdrn_train_step_features, lbdrn_train_group_size, lbdrn_train_workspace), to the library.
Shapes, feature configurations and the float64 step are those of tests/train_plan_reference.py and tests/train_step_f64.py.

An instance of k_train_half is (LQ, NL, NT): the quarter length of layer 0, the hidden layers, bc / 16.  k_dw_wide<NT, NL>
follows from it."""
import functools
import os
import re

import numpy as np

import train_plan_reference as R

WIDE_SOURCE = os.path.join(R.CSRC, "train_wide.inc")

# ---------------------------------------------------------------------------------------------------------------------
# the intended values (tests/test_wide_plan_host.py asserts that the sources state the same)

LQS = (16, 32, 48, 52, 64)                          # make_wide_plan's list, in the order it is walked
WAVE_XP = {16: 80, 32: 144, 48: 208, 52: 208, 64: 272}   # row pitch of the row matrix = LDS row pitch (train_mfma.hip: wave_xp)
BCS = (128, 256)
NLS = (1, 2)
DW_KS = 1024                                        # samples per slice of k_dw_wide
HB = 32                                             # rows per workgroup of k_train_half
WOP = 16                                            # channel slots of dz_out
GRAD_SLICE, LOSS_BLOCKS = 256, 64                   # generic.hip: the generic step's workspace (lbdrn_train_workspace is the larger of the two)
LDS_BOUND = 160 * 1024
MAX_C = 16
HALF_INSTANCES = tuple((lq, nl, nt) for lq in LQS for nl in NLS for nt in (8, 16))   # k_train_half<LQ, NL, NT>
DW_INSTANCES = tuple((nt, nl) for nt in (16, 8) for nl in NLS)                      # k_dw_wide<NT, NL>


def _read(path):
    with open(path) as f:
        return f.read()


def source_constants():
    """The same constants and dispatch cases as csrc/train_wide.inc, train_mfma.hip and generic.hip state them."""
    w, m, g = _read(WIDE_SOURCE), _read(R.TRAIN_SOURCE), _read(os.path.join(R.CSRC, "generic.hip"))
    k = {}
    lqs, = re.findall(r"for \(int lq : \{([\d, ]+)\}\)\n\s+if \(p\.fm\.Fe <= 4 \* lq && p\.RP <= wave_xp\(lq\)\)", w)
    k["LQS"] = tuple(int(x) for x in lqs.split(","))
    xp, = re.findall(r"constexpr int wave_xp\(int LQ\) \{ return LQ == 16 \? (\d+) : LQ == 32 \? (\d+) : LQ == 48 \|\| LQ == 52 \? (\d+) : (\d+); \}", m)
    k["WAVE_XP"] = {16: int(xp[0]), 32: int(xp[1]), 48: int(xp[2]), 52: int(xp[2]), 64: int(xp[3])}
    for name, text in (("DW_KS", w), ("HB", w), ("WOP", m), ("GRAD_SLICE", g), ("LOSS_BLOCKS", g)):
        found = re.findall(r"constexpr int %s = (\d+);" % name, text)
        assert len(found) == 1, (name, found)
        k[name] = int(found[0])
    bound, = re.findall(r"if \(\(size_t\)p\.lds_floats \* 4 > (\d+) \* 1024\) return false;", w)
    k["LDS_BOUND"] = int(bound) * 1024
    # dispatch_wide: a case per LQ (the last one as `default`), dispatch_wide_lq: NL 1 / 2 x NT 16 / 8
    cases = re.findall(r"case (\d+): return dispatch_wide_lq<(\d+)>\(A, nwg, s, configure\);", w)
    assert all(a == b for a, b in cases)
    default, = re.findall(r"default: return dispatch_wide_lq<(\d+)>\(A, nwg, s, configure\);", w)
    lq_cases = tuple(int(a) for a, _ in cases) + (int(default),)
    inner = re.findall(r"launch_wide<LQ, (\d), (\d+)>\(A, nwg, s, configure\)", w)
    assert "if (A.p.NT == 16) return one ?" in w and "const bool one = A.net.nl == 1;" in w
    k["HALF_INSTANCES"] = tuple(sorted((lq, int(nl), int(nt)) for lq in lq_cases for nl, nt in inner))
    k["DW_INSTANCES"] = tuple((int(nt), int(nl)) for nt, nl in re.findall(r"k_dw_wide<(\d+), (\d)><<<grid, WAVE_THREADS, 0, s>>>\(A\)", w))
    # how the plan and the geometry are read
    for line in ("if (net.act != LBDRN_ACT_SINE || (net.bc != 128 && net.bc != 256) || net.nl < 1 || net.nl > 2 || net.C > 16 || net.F < 1) return false;",
                 "p.RP = (p.fm.Fe + net.C + 3) / 4 * 4;", "p.NT0 = (p.fm.Fe + 15) / 16;", "if (16 * p.NT0 > wave_xp(p.LQ)) return false;",
                 "p.xo = (16 * p.NT0 + 63) / 64 * 64;", "if (p.xo > 256) return false;", "p.slab_floats = (s + 127) / 128 * 128;",
                 "const int ep = net.bc + 4, r0 = std::max(HB * wave_xp(p.LQ), HB * ep);",
                 "p.lds_floats = r0 + (net.nl > 1 ? HB * ep : 0) + 2 * HB * 20 + 4;",
                 "const int T0 = UM * IM0, T1 = NL > 1 ? UM * UM : 0, T = T0 + T1 + 1;",
                 "const int ns_x = (A.nslices - xcd + 7) >> 3;", "const unsigned grid = 8u * (unsigned)(ns_max * T);",
                 "Dw.nrows = (nwg * rpw + 63) / 64 * 64;", "if (wg == (int)gridDim.x - 1 && (gridDim.x & 1)) {"):
        assert w.count(line) == 1, line
    assert "if (count != 1) { set_error(\"groups of fits run on the bc = 64 fused step only\"); return LBDRN_E_UNSUPPORTED; }" in m
    return k


# ---------------------------------------------------------------------------------------------------------------------
# the plan, the workspace and one step's launches

def plan(shape, bc):
    """make_wide_plan -> None (no fused step at this width) or dict(LQ, Fe, RP, NT0, NT, xo, pack_floats, slab_floats, lds_floats)."""
    nl, C, F = shape.nl, shape.C, shape.F
    if shape.act != "sine" or bc not in BCS or nl not in NLS or C > MAX_C or F < 1:
        return None
    Fe = R.centre_skipping_fe(shape.colors, shape.relative, shape.P, C, shape.D, F)
    RP = (Fe + C + 3) // 4 * 4
    LQ = next((lq for lq in LQS if Fe <= 4 * lq and RP <= WAVE_XP[lq]), 0)
    if not LQ:
        return None
    NT0 = (Fe + 15) // 16
    if 16 * NT0 > WAVE_XP[LQ]:
        return None
    RP, NT = WAVE_XP[LQ], bc // 16
    pack = NT * LQ * 64 + 2 * (nl - 1) * NT * NT * 256 + 2 * NT * 256
    s = NT * NT0 * 256 + (nl - 1) * NT * NT * 256 + NT * 256 + nl * bc + 16
    slab = (s + 127) // 128 * 128
    xo = (16 * NT0 + 63) // 64 * 64
    ep = bc + 4
    lds = max(HB * WAVE_XP[LQ], HB * ep) + (HB * ep if nl > 1 else 0) + 2 * HB * 20 + 4
    if lds * 4 > LDS_BOUND or xo > 256:
        return None
    return dict(LQ=LQ, Fe=Fe, RP=RP, NT0=NT0, NT=NT, xo=xo, pack_floats=pack, slab_floats=slab, lds_floats=lds)


def instance(shape, bc):
    """(LQ, NL, NT) of the k_train_half that steps the shape, or None."""
    p = plan(shape, bc)
    return None if p is None else (p["LQ"], shape.nl, p["NT"])


def _al(x):
    return (x + 255) // 256 * 256


def wide_workspace_bytes(shape, bc, H, W, bs):
    """wide_ws_layout(...).total"""
    p = plan(shape, bc)
    nwg = (bs + HB - 1) // HB
    nrows = (nwg * HB + 63) // 64 * 64
    nslabs = (nrows + DW_KS - 1) // DW_KS
    o = _al(H * W * p["RP"] * 4) + _al(p["pack_floats"] * 4) + _al(nslabs * p["slab_floats"] * 4) + _al(nwg * 8)
    o += _al(p["slab_floats"] * 4 * 4)
    o += _al(nrows * p["xo"] * 4) + 2 * shape.nl * _al(nrows * bc * 4) + _al(nrows * WOP * 4)
    return o


def generic_workspace_bytes(shape, bc, bs):
    """generic.hip: carve_train -- what the generic step of the same net asks for"""
    nl, C, F = shape.nl, shape.C, shape.F
    act = nl * bs * bc * 4
    np_ = sum((bc if l < nl else C) * ((F if l == 0 else bc) + 1) for l in range(nl + 1))
    nsl = (bs + GRAD_SLICE - 1) // GRAD_SLICE
    return (2 * _al(act) + 2 * _al(bs * C * 4) + 2 * _al(bs * bc * 4) + _al(np_ * 4) + _al(nsl * max(bc, C) * (max(bc, F) + 1) * 4)
            + _al(LOSS_BLOCKS * 8) + _al(bs * F * 4) + _al(bs * C * 4))


def workspace_bytes(shape, bc, H, W, bs):
    """lbdrn_train_workspace: one buffer serves either path, so it is the larger of the two"""
    g = generic_workspace_bytes(shape, bc, bs)
    return max(g, wide_workspace_bytes(shape, bc, H, W, bs)) if plan(shape, bc) else g


def launches(shape, bc, B):
    """One step of B rows: the geometry of k_train_half and k_dw_wide."""
    p = plan(shape, bc)
    nwg = (B + HB - 1) // HB
    nrows = (nwg * HB + 63) // 64 * 64
    nslices = (nrows + DW_KS - 1) // DW_KS
    UM, IM0 = p["NT"] // 4, (p["NT0"] + 3) // 4
    T = UM * IM0 + (UM * UM if shape.nl > 1 else 0) + 1
    last = nrows - DW_KS * (nslices - 1)
    return dict(nwg=nwg, nrows=nrows, nslices=nslices, tasks=T, grid=8 * ((nslices + 7) // 8) * T, IM0=IM0,
                part_strip_block=p["NT0"] % 4 != 0,                 # the last block of four strips of dW_0 is part-filled
                zero_fill=nwg % 2 == 1,                             # the last workgroup zero-fills rows nwg * 32 .. nrows
                part_workgroup=B % HB != 0,
                idle_waves=4 - (last + DW_KS // 4 - 1) // (DW_KS // 4),   # waves of the last slice without rows
                slices_per_xcd=tuple((nslices - x + 7) // 8 for x in range(8)))


# ---------------------------------------------------------------------------------------------------------------------
# the census

HEADLINE = (0, 0, 1, 1, 8, 2)                       # 8 bands, D = 2, relative colours: F 200, Fe 192 (BASELINE configs[2])
BOUNDARIES = ((64, 65), (128, 129), (192, 193), (208, 209))   # Fe <= 4 LQ: 16|32|48|52|64
BUMPED = ((1, 1, 1, 0, 16, 1), (1, 0, 1, 0, 8, 2))  # C16 D1 cek- F194 and C8 D2 c-k- F202: RP 212 > 208, so LQ 64 and not 52


@functools.lru_cache(maxsize=None)
def planned_shapes(nl=2, bc=256):
    """the real shapes with a wide plan, smallest first"""
    return tuple(s for s in R.shapes(nl, "sine") if plan(s, bc) is not None)


@functools.lru_cache(maxsize=None)
def reachable_fe():
    return tuple(sorted({s.Fe for s in planned_shapes()}))


def nearest(side, edge):
    fe = reachable_fe()
    return max(f for f in fe if f <= edge) if side == "lo" else min(f for f in fe if f >= edge)


class Row:
    """One census row: a shape at a width, the k_train_half instance that steps it, and why the row is in the table."""

    def __init__(self, shape, bc, why):
        self.shape, self.bc, self.why = shape, bc, why
        p = plan(shape, bc)
        self.p, self.Fe, self.NT0, self.LQ = p, p["Fe"], p["NT0"], p["LQ"]
        self.inst = (p["LQ"], shape.nl, p["NT"])
        self.dw = (p["NT"], shape.nl)
        sw = "".join(c if on else "-" for c, on in zip("cekr", (shape.coords, shape.embed, shape.colors, shape.relative)))
        self.id = f"half-LQ{self.LQ}-nl{shape.nl}-bc{bc}-Fe{self.Fe}-C{shape.C}D{shape.D}{sw}"

    def key(self):
        return (self.shape.key(), self.shape.coords, self.shape.embed, self.bc)


@functools.lru_cache(maxsize=None)
def census():
    """-> (rows, unreachable): one Row per k_train_half instance at its smallest real shape, then -- at bc = 256, nl = 2 -- the
    class boundaries of Fe, the two shapes the row pitch pushes to LQ 64, the largest Fe, a full and a part-filled last strip
    per LQ and every residue of NT0 mod 4; unreachable = the built instances no real shape selects (there are none)."""
    rows, unreachable, seen = [], [], {}

    def push(shape, bc, why):
        r = Row(shape, bc, why)
        if r.key() in seen:
            seen[r.key()].why += "; " + why             # one row, every reason it is in the table
        else:
            seen[r.key()] = r
            rows.append(r)

    for lq, nl, nt in HALF_INSTANCES:
        s = next((s for s in R.shapes(nl, "sine") if instance(s, 16 * nt) == (lq, nl, nt)), None)   # (shapes() is sorted by Shape.size)
        if s is None:
            unreachable.append((lq, nl, nt))
        else:
            push(s, 16 * nt, "instance")
    by_fe = lambda fe: next(s for s in planned_shapes() if s.Fe == fe)
    for lo, hi in BOUNDARIES:
        push(by_fe(nearest("lo", lo)), 256, f"boundary {lo}|{hi}, below")
        push(by_fe(nearest("hi", hi)), 256, f"boundary {lo}|{hi}, above")
    for cfg in BUMPED:
        push(R.Shape(*cfg, 2, "sine"), 256, "row pitch 212 > 208: LQ 64, not 52")
    push(by_fe(reachable_fe()[-1]), 256, "largest Fe")
    wide = lambda: [r for r in rows if r.bc == 256 and r.shape.nl == 2]
    for lq in LQS:
        for full in (True, False):
            if not any(r.LQ == lq and (r.Fe % 16 == 0) == full for r in wide()):
                s = next((s for s in planned_shapes() if plan(s, 256)["LQ"] == lq and (s.Fe % 16 == 0) == full), None)
                if s is not None:
                    push(s, 256, f"LQ {lq}: a last strip that is {'full' if full else 'part-filled'}")
    for res in range(4):
        if not any(r.NT0 % 4 == res for r in wide()):
            push(next(s for s in planned_shapes() if plan(s, 256)["NT0"] % 4 == res), 256, f"NT0 = {res} mod 4")
    return tuple(rows), tuple(unreachable)


def table_text():
    rows, _ = census()
    lines = ["| row | shape | bc | F | Fe | LQ | NT0 | IM0 | why |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| `{r.id}` | {r.shape!r} | {r.bc} | {r.shape.F} | {r.Fe} | {r.LQ} | {r.NT0} | {(r.NT0 + 3) // 4} | {r.why} |")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of a row and the float64 epoch they are compared with

H, W, K = R.H, R.W, R.K      # 13 x 11 = 143 pixels, K = 5, H, W > D
BIG_H, BIG_W = 96, 97        # 9,312 pixels: 33 workgroups and 2 slices at bs = 1040, 291 workgroups and 10 slices at bs = 9312
BS_ODD = 90                  # 90 + 53 rows: three workgroups (odd: a zero-filled half block, the last part-filled), then two
BS_STALE = 128               # 128 + 15 rows: one workgroup after four -- rows 32..63 held the first step's dz
BS_TAIL = R.BS_TAIL          # 71, 71, 1: a one-row tail


def init_params(rng, F, C, nl, bc):
    """train_plan_reference.init_params (uniform weights at the reference's Sine scales) at a hidden width of bc"""
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = 1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


def fit_inputs(shape, bc, seed, fit, h=H, w=W):
    """Image, initial parameters and permutation of fit `fit` of a row: all three differ between the fits, and so does the
    largest MSB value (fit k draws k + 9 bits)."""
    rng = np.random.default_rng([seed, fit, shape.F, shape.C, shape.nl, bc, h, w])
    img = rng.integers(0, 1 << (9 + fit), (shape.C, h, w)).astype(np.uint16)
    img[0, 0, 0] |= np.uint16(1 << (8 + fit))          # the largest MSB value is that of the fit's bit count
    p0 = init_params(rng, shape.F, shape.C, shape.nl, bc)
    perm = rng.permutation(h * w).astype(np.int64)
    return img, p0, perm


def features_and_labels_f64(shape, img):
    """the oracle's features and labels of every pixel, as float64"""
    import oracle as O
    msb, lab, mx = O.split_bits(img, K)
    ocfg = O.FeatCfg(shape.coords, shape.embed, 1.4, 12, shape.colors, shape.relative)
    return O.features(msb, shape.D, ocfg, mx).astype(np.float64), lab.astype(np.float64)


def zero_lr_epoch_f64(shape, bc, x, t, p0, perm, bs):
    """An epoch at lr = 0 from zero moments, in float64: the parameters never move, so every step's gradient is taken at p0.
    -> (losses [S], exp_avg, exp_avg_sq, [gradient of step s])"""
    import train_step_f64 as T
    p = p0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    losses, grads = [], []
    for first in range(0, len(perm), bs):
        b = perm[first:first + bs]
        loss, g = T.loss_and_grad_f64(p, x[b], t[b], shape.F, bc, shape.C, shape.nl, "sine")
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        losses.append(loss)
        grads.append(g)
    return np.array(losses), m, v, grads


def blocks(shape, bc):
    """[(name, slice)] of the flat parameter vector: W_0, b_0, (W_1, b_1,) W_last, b_last"""
    import train_step_f64 as T
    out = []
    for l, (w, _, b) in enumerate(T.layer_slices(shape.F, bc, shape.C, shape.nl)):
        name = "last" if l == shape.nl else str(l)
        out += [(f"W_{name}", w), (f"b_{name}", b)]
    return out
