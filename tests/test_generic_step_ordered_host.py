"""The ordered float32 restatement of the generic training step (oracle/lbdrn_oracle.c: orc_step_ordered) by itself,
without a device: it is a training step (float64 bounds), its inputs can tell the kernels' order from its neighbours'
(every mutation changes gradient bits), and no row leaves the range in which float32 arithmetic is the same everywhere
(no subnormal, no non-finite value).  tests/test_gpu_generic_step_bits.py then holds the kernels to it bit for bit."""
import numpy as np
import pytest

import oracle as O
import train_step_f64 as T
from generic_step_rows import (KINK, LR, MIN_MAGNITUDE, ROWS, blind_mutations, first_good_seed, first_step, inputs,
                               kink_margin, mutations, ordered_step, same_bits)

LOSS_BOUND, GRAD_BOUND = 1e-5, 2e-5     # the project's training bounds: relative loss, share of the largest gradient entry
IDS = [r.name for r in ROWS]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_ordered_step_is_within_the_training_bounds_of_float64(row):
    p0, x, t, _ = inputs(row)
    loss64, g64 = T.loss_and_grad_f64(p0.astype(np.float64), x.astype(np.float64), t.astype(np.float64), row.F, row.bc,
                                      row.C, row.nl, row.act)
    got = first_step(row)
    print(row.name, "loss", abs(float(got["loss"]) - loss64) / loss64, "grads", np.abs(got["grads"] - g64).max() / np.abs(g64).max())
    assert abs(float(got["loss"]) - loss64) <= LOSS_BOUND * loss64
    assert np.abs(got["grads"] - g64).max() <= GRAD_BOUND * np.abs(g64).max()


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_three_ordered_adam_steps_agree_with_the_float64_sum_oracle(row):
    """orc_train_step (float64 gradient sums, the same Adam lines), three steps, each from the state the ordered step
    is in (teacher-forced: two float32 trajectories of a deep Sine net drift apart by more than a step's rounding, which
    says nothing about either step): loss, gradient and first moment of every step within the training bounds, the
    parameters within 2e-5 of their norm (the bound the epoch tests hold a float32 run's parameters to).  Steps 2 and 3
    meet nonzero moments and the bias corrections of their step counts."""
    p0, x, t, _ = inputs(row)
    state = (p0.copy(), np.zeros_like(p0), np.zeros_like(p0))
    for step in (1, 2, 3):
        po, mo, vo = (a.copy() for a in state)
        got = ordered_step(row, step=step, state=state)
        state = (got["params"], got["exp_avg"], got["exp_avg_sq"])
        with O.hidden_activation(row.act):
            lo, go = O.train_step(po, mo, vo, row.F, row.bc, row.C, row.nl, x, t, LR, step)
        assert abs(float(got["loss"]) - lo) <= LOSS_BOUND * lo, step
        assert np.abs(got["grads"] - go).max() <= GRAD_BOUND * np.abs(go).max(), step
        assert np.abs(got["exp_avg"] - mo).max() <= GRAD_BOUND * np.abs(mo).max(), step
        assert np.linalg.norm(got["params"] - po) <= 2e-5 * np.linalg.norm(po), step


@pytest.mark.parametrize("row", [r for r in ROWS if r.B <= 256 and r.B % 16 == 0], ids=lambda r: r.name)
def test_head_bias_gradient_is_a_running_float32_sum(row):
    """One slice of whole k-tiles: db of the head is fmaf(dz, 1, acc) from +0 over the batch, a plain sequential sum."""
    p0, x, t, _ = inputs(row)
    with O.hidden_activation(row.act):
        y = O.forward(p0, row.F, row.bc, row.C, row.nl, x)
    inv = np.float32(1) / (np.float32(row.B) * np.float32(row.C))
    dz = ((np.float32(2) * (y - t)) * inv) * (y * (np.float32(1) - y))
    assert dz.dtype == np.float32
    acc = np.zeros(row.C, np.float32)
    for b in range(row.B):
        acc = acc + dz[b]
    assert acc.dtype == np.float32
    assert same_bits(first_step(row)["grads"][-row.C:], acc)


def test_the_head_bias_check_has_rows():
    assert [r.name for r in ROWS if r.B <= 256 and r.B % 16 == 0] == ["T4"]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_inputs_tell_the_kernels_order_from_its_neighbours(row):
    names = [n for n, _, _ in mutations(row)]
    assert "last row dropped from the last slice" in names
    assert ("slices of 128 rows" in names) == (row.B > 128)
    assert ("slices added in reverse" in names) == (row.B > 512)
    assert ("v * (cos * 30)" in names) == (row.act == "sine")
    assert blind_mutations(row, row.seed) == []


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_seed_is_the_first_that_suits_the_row(row):
    assert first_good_seed(row) == row.seed
    if row.act == "relu":
        assert kink_margin(row, row.seed) >= KINK


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_no_intermediate_leaves_the_normal_range(row):
    smallest, nonfinite = ordered_step(row, want_range=True)["range"]
    print(row.name, "smallest nonzero magnitude 2^%.1f" % np.log2(smallest), "non-finite", nonfinite)
    assert nonfinite == 0
    assert smallest >= MIN_MAGNITUDE


def test_backward_ordered_of_the_mse_gradient_is_the_ordered_step():
    """dy = (2 (y - t)) * inv formed in float32 as the head forms it: the autograd entry gives the step's gradient bits."""
    for row in (ROWS[0], ROWS[2]):
        p0, x, t, _ = inputs(row)
        with O.hidden_activation(row.act):
            y = O.forward(p0, row.F, row.bc, row.C, row.nl, x)
            inv = np.float32(1) / (np.float32(row.B) * np.float32(row.C))
            yo, grads, dx = O.backward_ordered(p0.copy(), row.F, row.bc, row.C, row.nl, x, (np.float32(2) * (y - t)) * inv)
        assert same_bits(yo, y)
        assert same_bits(grads, first_step(row)["grads"])
        assert dx.shape == (row.B, row.F) and np.isfinite(dx).all()
