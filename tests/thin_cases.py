"""The shared case table of the thin-raster and dark-tile tests (tests/test_thin_rasters_host.py on the CPU,
tests/test_gpu_thin_rasters.py and tests/test_gpu_dark_tiles.py on the device).

A raster is THIN where H <= D or W <= D: numpy's reflect padding then folds more than once (or, on an axis of one pixel,
repeats it), and the kernels leave their one-reflection code: the dividing staging branch of k_apply_mfma, reflect_idx
behind reflect_fast (k_apply_wide, both row builders), and k_build_rows in place of k_build_rows_tiled.  `encode.py -sr 3`
on a 7 x 5 scene makes such tiles (2x1, 3x1, 2x3, 3x3, w x h) on its first split.

Shapes are written H x W.  Images are uniform 16-bit noise at K = 5 (MSB values 0..2047, independent per pixel): a wrong
neighbour index changes a feature by O(1).  A DARK image has every sample below 2^K: its MSB plane is zero everywhere
(msb_max == 0), which the library normalises by 1 (include/lbdrn_hip.h, at msb_max).

A plain module: no fixture, no marker, no device."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

K = 5

# (H, W, D) per group of the table; D is chosen so that every shape is thin and, over the table, D = 1, 2 and 3 all occur
# and an axis of 2 <= n <= D (reflection folds more than once) occurs in either direction
SHAPES = (
    ("1x1", ((1, 1, 1), (1, 1, 3))),
    ("row", ((1, 2, 2), (1, 3, 3), (1, 7, 2), (1, 70, 1))),
    ("column", ((2, 1, 2), (3, 1, 3), (7, 1, 2), (70, 1, 1))),
    ("both", ((2, 2, 2), (2, 2, 3), (2, 3, 2), (3, 2, 2), (3, 3, 3))),
    ("tile-edge", ((2, 65, 2), (3, 130, 3), (2, 33, 2), (130, 2, 2))),     # one thin axis, the other across the 64-column tile edge
)
FILL = (5, 7, 2)                  # not thin, but N = 35 < 64: for the workgroup-fill cases of the training side only
BANDS = (1, 2, 8)
WIDE_BANDS_ROW = (16, 1, 70, 1)  # the one C = 16 row: (C, H, W, D)
MAX_PIXELS = 390                  # 3 x 130, the largest raster of the table


class Case:
    """One row: bands, raster, window, feature switches."""

    def __init__(self, C, H, W, D, relative=True, coords=False, embed=False):
        self.C, self.H, self.W, self.D = C, H, W, D
        self.relative, self.coords, self.embed = bool(relative), bool(coords), bool(embed)
        self.P = 0 if not coords else (25 if embed else 1)
        self.F = 2 * self.P + C * (2 * D + 1) ** 2
        self.N = H * W
        self.thin = H <= D or W <= D
        self.id = f"C{C}-{H}x{W}-D{D}-" + ("rel" if relative else "abs") + ("-embed" if embed else "-coords" if coords else "")

    def cfg(self, activation="sine"):
        from lbdrn_hip.features import FeatCfg
        return FeatCfg(self.coords, self.embed, 1.4, 12, True, self.relative, activation)

    def ocfg(self):
        import oracle as O
        return O.FeatCfg(self.coords, self.embed, 1.4, 12, True, self.relative)

    def image(self):
        return noise_image(self.C, self.H, self.W)

    def __repr__(self):
        return self.id


def noise_image(C, H, W, seed=0):
    rng = np.random.default_rng([seed, C, H, W])
    return rng.integers(0, 1 << 16, (C, H, W)).astype(np.uint16)


def dark_image(C, H, W, seed=0):
    """every sample below 2^K: the MSB plane is zero everywhere, the labels are noise"""
    rng = np.random.default_rng([seed, C, H, W, K])
    return rng.integers(0, 1 << K, (C, H, W)).astype(np.uint16)


def _cases():
    """Every shape at every band count with relative and with absolute colours; where both axes have two pixels or more also
    with coordinates alone (P = 1, relative colours), with coordinates and embedding (P = 25) on relative and on absolute
    colours.  A network whose weights the fused apply pass cannot hold at a row's feature count (fused_apply_takes: bc = 128
    ReLU from about 200 features on, on any raster) is refused there, which the GPU test asserts."""
    out = []
    for _, shapes in SHAPES:
        for H, W, D in shapes:
            for C in BANDS:
                out += [Case(C, H, W, D, True), Case(C, H, W, D, False)]
                if H >= 2 and W >= 2:                 # an axis of one pixel has no coordinate to speak of: position 0 (AXIS_CASES)
                    out += [Case(C, H, W, D, True, True, False), Case(C, H, W, D, True, True, True), Case(C, H, W, D, False, True, True)]
    C, H, W, D = WIDE_BANDS_ROW
    out += [Case(C, H, W, D, True), Case(C, H, W, D, False)]
    return tuple(out)


CASES = _cases()                       # every row is thin
AXIS_CASES = tuple(Case(C, H, W, D, True, True, embed) for C, H, W, D, embed in
                   ((2, 1, 7, 2, True), (2, 7, 1, 2, False), (1, 1, 1, 1, True)))   # coordinates on an axis of ONE pixel: position 0
DARK_SHAPES = ((4, 9, 12, 2), (2, 1, 7, 2))                                         # (C, H, W, D) of the dark-tile tests

assert all(c.thin and c.N <= MAX_PIXELS for c in CASES)


# ---------------------------------------------------------------------------------------------------------------------
# networks of the apply side, and which of them the fused apply pass takes

NETWORKS = tuple((bc, nl, act) for bc in (32, 64, 128) for act in ("sine", "relu") for nl in (1, 2)) + \
           ((256, 1, "sine"), (256, 2, "sine"))


def rand_params(rng, F, bc, C, nl, gain=1.0):
    """SIREN-like magnitudes so that sin(30 z) wraps a few times (the draw of tests/test_gpu_parity.py)"""
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = (1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


def fused_apply_takes(C, D, P, F, bc, nl, act):
    """Whether LBDRN_PATH_MFMA has an apply kernel for this network on these features: make_plan (csrc/apply_mfma.hip: the
    weights of k_apply_mfma resident in 160 KB of LDS beside a one-row tile) or make_wapply_plan (csrc/apply_wide.inc: the
    streaming kernel, Sine, bc = 128 / 256, at most two hidden layers, a one-row tile in 64 KB).  Neither reads H or W: a
    thin raster is refused exactly where a large one of the same bands and window is.  The two planners are restated once, in
    tests/apply_plan_reference.py: this is its `supported` for a table row (colours on; P = 0, 1 or 25)."""
    import apply_plan_reference as R
    s = R.Shape(C, D, bc, nl, act, coords=P > 0, embed=P > 1)
    assert (s.P, s.F) == (P, F), (s, P, F)
    return R.supported(s)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of the colour block of the reference's feature matrix

def _index_map(n, D, mode):
    """source index of each of the n + 2 D padded positions of an axis of n pixels"""
    i = np.arange(-D, n + D)
    if mode == "edge":
        return np.clip(i, 0, n - 1)
    if mode == "onefold":           # one reflection, then clamped: right only where D < n
        r = np.abs(i)
        r = np.where(r >= n, 2 * (n - 1) - r, r)
        return np.clip(r, 0, n - 1)
    raise ValueError(mode)


def colour_features(msb, D, relative, mode="reflect"):
    """[H*W, C (2D+1)^2] float32: every band's plane divided by the largest MSB value, padded by D on either side, every
    pixel's (2D+1)^2 window in (band, dy, dx) order, minus the window's centre where `relative` and D > 0.  mode "reflect"
    is the reference's; "edge", "symmetric" (numpy.pad's) and "onefold" are the wrong paddings a kernel could implement."""
    C, H, W = msb.shape
    p = msb.astype(np.float32) / np.float32(msb.max())
    if mode in ("reflect", "symmetric"):
        padded = np.pad(p, ((0, 0), (D, D), (D, D)), mode=mode)
    else:
        padded = p[:, _index_map(H, D, mode)][:, :, _index_map(W, D, mode)]
    side = 2 * D + 1
    win = np.lib.stride_tricks.sliding_window_view(padded, (side, side), axis=(1, 2))      # [C, H, W, side, side]
    if relative and D > 0:
        win = win - p[:, :, :, None, None]
    return np.ascontiguousarray(win.transpose(1, 2, 0, 3, 4).reshape(H * W, C * side * side), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the training side: one row per kernel family on a thin raster (the step runs behind k_build_rows), and 5 x 7 for N < 64

class TrainRow:
    """name, the kernel the row is about, network (bc, nl, act), features (C, D, coords + embedding), raster, alone hint"""

    def __init__(self, name, kernel, bc, nl, act, C, D, H, W, embed=False, alone=False, seed=0):
        self.id, self.kernel, self.bc, self.nl, self.act = name, kernel, bc, nl, act
        self.case = Case(C, H, W, D, True, embed, embed)
        self.C, self.D, self.H, self.W, self.alone, self.seed = C, D, H, W, alone, seed
        self.F, self.N = self.case.F, H * W
        # relative colours, D > 0: the fused steps leave the window centres out (the nl = 3 tile kernel multiplies them)
        self.Fe = self.F if kernel == "k_train_mfma" else self.F - C

    def shape(self):
        """the row as tests/train_plan_reference.py and tests/wide_plan_reference.py state a shape"""
        import train_plan_reference as R
        return R.Shape(self.case.coords, self.case.embed, True, True, self.C, self.D, self.nl, self.act)

    def group_size(self):
        """fits the library steps in one launch: 4 on k_train_stream / k_train_split, 1 on the tile kernel and at bc >= 128"""
        return 4 if self.kernel in ("k_train_stream", "k_train_split") else 1

    def __repr__(self):
        return self.id


TRAIN_ROWS = (
    TrainRow("stream-nl1-sine-1x70", "k_train_stream", 64, 1, "sine", 8, 1, 1, 70),
    TrainRow("stream-nl2-sine-2x33", "k_train_stream", 64, 2, "sine", 8, 2, 2, 33),
    TrainRow("stream-nl1-relu-3x3", "k_train_stream", 64, 1, "relu", 1, 3, 3, 3, seed=2),   # (seed: reference_chain's condition)
    TrainRow("stream-nl2-relu-2x33", "k_train_stream", 64, 2, "relu", 2, 2, 2, 33),
    TrainRow("split-LQ24-2x33", "k_train_split", 64, 2, "sine", 4, 2, 2, 33, alone=True),
    TrainRow("split-LQ48-1x70", "k_train_split", 64, 2, "sine", 8, 2, 1, 70, alone=True),
    TrainRow("split-LQ64-embed-2x33", "k_train_split", 64, 2, "sine", 8, 2, 2, 33, embed=True, alone=True),
    TrainRow("split-LQ96-3x3", "k_train_split", 64, 2, "sine", 8, 3, 3, 3, alone=True),
    TrainRow("split-LQ96-2x33", "k_train_split", 64, 2, "sine", 8, 3, 2, 33, alone=True),
    TrainRow("tile-nl3-1x70", "k_train_mfma", 64, 3, "sine", 2, 2, 1, 70),
    TrainRow("half-bc128-2x33", "k_train_half", 128, 2, "sine", 8, 2, 2, 33),
    TrainRow("half-bc256-1x70", "k_train_half", 256, 2, "sine", 8, 2, 1, 70),
    TrainRow("half-bc256-nl1-3x3", "k_train_half", 256, 1, "sine", 2, 3, 3, 3),
    TrainRow("stream-nl2-sine-5x7", "k_train_stream", 64, 2, "sine", 8, 2, 5, 7),          # N = 35 < 64, not thin
    TrainRow("split-LQ48-5x7", "k_train_split", 64, 2, "sine", 8, 2, 5, 7, alone=True),
)
TINY = ((1, 1), (1, 2), (1, 3))       # N = 1, 2, 3: whole fits
BS_FIRST = 100                        # the first step takes min(100, N) rows: the whole raster, one or two workgroups
BATCH_SIZES = (64, 100, 1)            # one part-filled workgroup (N < 64) or a full one and a tail of 2 / 6 rows; one short minibatch
                                      # (100 > N); N one-row minibatches
LR_FIT, LR_CHAIN = 1e-3, 1e-4         # learning rates of the two-epoch chains whose losses two paths are compared on (chain_lr)
LONG_CHAIN = 8                        # steps from which a two-epoch chain runs at LR_CHAIN
CHAIN_RTOL, CHAIN_OWN = 5e-5, 5e-6    # the bound on fused against generic losses, and what the reference's own chain may use of it
KINK = 1e-5                           # ReLU: no hidden pre-activation of the float64 step within this of 0 (tests/train_plan_reference.py)


def init_params(rng, F, bc, C, nl, act):
    """uniform weights at the reference's scales, the ReLU net's ten times larger (tests/train_plan_reference.py)"""
    return rand_params(rng, F, bc, C, nl, 10.0 if act == "relu" else 1.0)


def train_inputs(row, seed=None):
    """-> (image, initial parameters, permutation of the N pixels)"""
    seed = row.seed if seed is None else seed
    rng = np.random.default_rng([seed, row.F, row.C, row.nl, row.bc, row.N])
    img = rng.integers(0, 1 << 16, (row.C, row.H, row.W)).astype(np.uint16)
    p0 = init_params(rng, row.F, row.bc, row.C, row.nl, row.act)
    perm = rng.permutation(row.N).astype(np.int64)
    return img, p0, perm


def first_step_f64(row, img, p0, perm, B=BS_FIRST):
    """The first minibatch (the first min(B, N) pixels of perm) in float64 on the oracle's features and labels:
    -> (x, t, batch, loss, gradient)"""
    import oracle as O
    import train_step_f64 as T
    msb, lab, mx = O.split_bits(img, K)
    x = O.features(msb, row.D, row.case.ocfg(), mx)
    b = perm[:B]
    loss, g = T.loss_and_grad_f64(p0.astype(np.float64), x[b].astype(np.float64), lab[b].astype(np.float64), row.F, row.bc, row.C,
                                  row.nl, row.act)
    return x, lab, b, loss, g


def kink_free(row, p0, xb):
    import train_step_f64 as T
    return row.act != "relu" or T.kink_margin(p0, xb, row.F, row.bc, row.C, row.nl) >= KINK


def chain_lr(row, bs):
    """The fit's own rate where two epochs are a handful of steps (bs = 64 and 100: two or four), LR_CHAIN where they are a long
    chain (bs = 1: 18 to 140 steps): see reference_chain."""
    return LR_FIT if 2 * ((row.N + bs - 1) // bs) < LONG_CHAIN else LR_CHAIN


def reference_chain(row, bs, lr=None, epochs=2):
    """Two epochs of minibatches of bs rows, once in the generic path's own float32 arithmetic (oracle.train_step_ordered: the
    generic kernels bit for bit) and once in float64: -> (losses of every step, float32 chain; the same, float64).

    Why long chains run at LR_CHAIN (chain_lr): a chain of Adam steps amplifies rounding.  At lr = 1e-3 the 132 to 140 one-row steps of
    two epochs on a 66- or 70-pixel raster carry the generic path itself 1e-2 to 6.5e-1 away from float64 -- any two correct
    float32 implementations part there, and a comparison of their losses at rtol 5e-5 measures the chain, not a kernel.  At
    1e-4 the generic path's own distance from float64 stays under CHAIN_OWN, a tenth of the bound, on every row and batch
    size (tests/test_thin_rasters_host.py asserts it, on the CPU), while two epochs still move every weight by about its
    own size, so that a wrong update shows in the second epoch's losses.  A row that missed the condition got another seed."""
    import oracle as O
    import train_step_f64 as T
    lr = chain_lr(row, bs) if lr is None else lr
    img, p0, perm = train_inputs(row)
    msb, lab, mx = O.split_bits(img, K)
    x = O.features(msb, row.D, row.case.ocfg(), mx)
    x64, t64 = x.astype(np.float64), lab.astype(np.float64)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    q = p0.astype(np.float64)
    qm, qv = np.zeros_like(q), np.zeros_like(q)
    l32, l64, step = [], [], 0
    with O.hidden_activation(row.act):
        for _ in range(epochs):
            for s in range(0, row.N, bs):
                b = perm[s:s + bs]
                step += 1
                l32.append(float(O.train_step_ordered(p, m, v, row.F, row.bc, row.C, row.nl, x[b], lab[b], lr, step)[0]))
                loss, _, q, qm, qv = T.train_step_f64(q, qm, qv, x64[b], t64[b], row.F, row.bc, row.C, row.nl, row.act, lr, step)
                l64.append(loss)
    return np.array(l32), np.array(l64)
