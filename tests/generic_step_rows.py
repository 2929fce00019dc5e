"""The fixed table of shapes the generic training step (csrc/generic.hip) is pinned at, bit for bit, to the ordered float32
restatement of the oracle (oracle/lbdrn_oracle.c: orc_step_ordered), with the inputs of every row.

The GEMM tile of generic.hip is 64 x 64 x 16, a GradW slice is 256 batch rows and k_reduce_slices adds the slices in
bodies of 16.  Every row is there for the edge named beside it; none is drawn.

A plain module: no fixture, no marker, no device.  tests/test_generic_step_ordered_host.py holds the inputs to their
conditions on the CPU; tests/test_gpu_generic_step_bits.py runs the kernels on them."""
import functools
from collections import namedtuple

import numpy as np

import oracle as O
import train_step_f64 as T

Row = namedtuple("Row", "name F bc C nl act B seed why")

LR = 1e-3
KINK = 1e-5          # tests/train_plan_reference.py: ReLU rows keep every hidden pre-activation this far from 0
MIN_MAGNITUDE = 2.0 ** -100

# seed: the first one at which first_good_seed()'s conditions hold (checked by the host test; stated here so that the GPU
# file does not search)
ROWS = (
    Row("T1", 200, 64, 8, 2, "sine", 300, 0, "the project's shape: GradW N = 65 and 201, the ones column alone in a tile; "
        "two slices, the second of 44 rows"),
    Row("T2", 1, 1, 1, 1, "sine", 1, 3, "every dimension 1: k-tiles of one term"),
    Row("T3", 3, 7, 2, 3, "relu", 63, 0, "k < 4, less than one MFMA step; M < 64; BackDx Kd = 2"),
    Row("T4", 15, 63, 3, 2, "sine", 256, 0, "GradW N = 64 = bc + 1: the ones column closes a full tile; one full slice"),
    Row("T5", 17, 65, 16, 2, "sine", 257, 0, "N = 66 and 18, M = 65, Kd = 17; the second slice has one row"),
    Row("T6", 33, 128, 17, 1, "relu", 513, 4, "full N tiles plus the ones column alone; three slices; BackDx Kd = 17"),
    Row("T7", 64, 129, 40, 4, "sine", 65, 0, "nl = 4; M = 129, N = 130; B just over a tile"),
    Row("T8", 5, 7, 2, 1, "sine", 3841, 0, "16 slices, the last of one row: the unrolled reduce body once, no remainder"),
    Row("T9", 5, 7, 2, 2, "sine", 4097, 0, "17 slices: the unrolled body plus a remainder of 1"),
    Row("T10", 6, 9, 3, 1, "relu", 8449, 6, "34 slices: two bodies plus a remainder of 2; the loss grid stride wraps"),
    Row("T11", 250, 256, 8, 2, "sine", 130, 0, "the wide shape on the generic path: Kd = 256, 16 k-tiles"),
    Row("T12", 16, 16, 1, 1, "sine", 15, 0, "one k-tile exactly; C = 1; B < 16"),
)
BY_NAME = {r.name: r for r in ROWS}


def init_params(rng, F, bc, C, nl, act):
    """uniform weights at the reference's scales (LBDRNmodel.py), the ReLU net's ten times larger -- init_params of
    tests/train_plan_reference.py at any bc"""
    gain = 10.0 if act == "relu" else 1.0
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = (1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(row, seed):
    rng = np.random.default_rng([seed, row.F, row.bc, row.C, row.nl, row.B])
    p0 = init_params(rng, row.F, row.bc, row.C, row.nl, row.act)
    x = rng.uniform(-1, 1, (row.B, row.F)).astype(np.float32)
    t = (rng.integers(0, 32, (row.B, row.C)).astype(np.float32) / np.float32(31)).astype(np.float32)
    dy = rng.standard_normal((row.B, row.C)).astype(np.float32)
    for a in (p0, x, t, dy):
        a.setflags(write=False)
    return p0, x, t, dy


def inputs(row, seed=None):
    """-> (params0, x [B,F] uniform in [-1, 1), t [B,C] = k / 31, dy [B,C] standard normal), read-only"""
    return _inputs(row, row.seed if seed is None else seed)


def ordered_step(row, seed=None, step=1, state=None, slice_rows=O.GRAD_SLICE, flags=0, want_range=False):
    """One ordered step of a row from (params, exp_avg, exp_avg_sq) = state (default: params0 and zero moments):
    -> dict(loss, grads, params, exp_avg, exp_avg_sq[, range])"""
    p0, x, t, _ = inputs(row, seed)
    p, m, v = (a.copy() for a in state) if state is not None else (p0.copy(), np.zeros_like(p0), np.zeros_like(p0))
    with O.hidden_activation(row.act):
        out = O.train_step_ordered(p, m, v, row.F, row.bc, row.C, row.nl, x, t, LR, step, slice_rows=slice_rows,
                                   flags=flags, want_range=want_range)
    res = dict(loss=np.float32(out[0]), grads=out[1], params=p, exp_avg=m, exp_avg_sq=v)
    if want_range:
        res["range"] = out[5]
    return res


@functools.lru_cache(maxsize=None)
def first_step(row):
    """the ordered first step of a row at its seed, computed once and shared (treat as read-only)"""
    return ordered_step(row)


def mutations(row):
    """(name, slice rows, flags) of every order the kernels do NOT use that this row's shape can tell from theirs"""
    out = []
    if row.B > 128:
        out.append(("slices of 128 rows", 128, 0))
    if row.B > 512:
        out.append(("slices added in reverse", O.GRAD_SLICE, O.REVERSE_SLICES))
    if row.act == "sine":
        out.append(("v * (cos * 30)", O.GRAD_SLICE, O.FACTOR_RIGHT))
    out.append(("last row dropped from the last slice", O.GRAD_SLICE, O.DROP_LAST_ROW))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def blind_mutations(row, seed):
    """the mutations that leave every gradient bit of the row's inputs at `seed` as it is"""
    base = ordered_step(row, seed)["grads"]
    return [name for name, sl, fl in mutations(row) if same_bits(ordered_step(row, seed, slice_rows=sl, flags=fl)["grads"], base)]


def kink_margin(row, seed):
    p0, x, _, _ = inputs(row, seed)
    return T.kink_margin(p0, x, row.F, row.bc, row.C, row.nl)


def first_good_seed(row, limit=64):
    """The rule every row's seed follows: the first seed at which (1) every mutation of mutations(row) changes at least
    one bit of the gradient -- inputs that cannot tell an order from the kernels' would let a kernel with that order
    pass -- and (2), ReLU rows, the float64 forward keeps every hidden pre-activation KINK away from 0, so that the row
    trains through live units (the forward bits are equal, so the kink cannot flip here)."""
    for seed in range(limit):
        if row.act == "relu" and kink_margin(row, seed) < KINK:
            continue
        if not blind_mutations(row, seed):
            return seed
    raise AssertionError(f"no seed below {limit} suits {row.name}")
