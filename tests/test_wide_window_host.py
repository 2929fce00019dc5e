"""Host-side facts of the wide fused training step (bc = 64, nl = 2, 256 < Fe <= 384: D = 3 windows on 6..8 bands with
relative colours), answered by the library without a GPU: the features the step multiplies, its workspace (the row matrix
in the step's order, 400 floats a pixel at 8 bands) and that its fits step in groups."""
import ctypes

import pytest

from lbdrn_hip import _lib, codec, ops
from lbdrn_hip.features import FeatCfg


def _shape(C, H, W, D, relative=True, act=ops.ACT_SINE, nl=2):
    g = _lib.Geom(C, H, W, 5, D, 100, 1, int(relative), 0, 0, None, None)
    F = C * (2 * D + 1) ** 2
    return g, _lib.Net(F, 64, C, nl, act)


def _q(name, g, net, *extra):
    return int(getattr(ops.lib(), name)(ctypes.byref(g), ctypes.byref(net), *extra))


@pytest.mark.parametrize("C", (6, 7, 8))
def test_step_features_skip_the_window_centres(C):
    g, net = _shape(C, 64, 64, 3)
    assert net.F == C * 49
    assert _q("lbdrn_train_step_features", g, net) == C * 48      # 8 bands: 384 of 392


def test_workspace_holds_the_row_matrix_in_the_wide_order():
    H = W = 2048
    bs = 8192
    g, net = _shape(8, H, W, 3)
    ws = _q("lbdrn_train_workspace", g, net, bs)
    rows = H * W * 400 * 4                                           # RP = 24 feature groups + 1 label group of 16 floats
    slabs = 4 * (bs // 32) * 29952 * 4                               # four rotating sets of 256 slabs of 117 KB (24 dW_0 strips)
    assert rows + slabs <= ws <= rows + slabs + (64 << 20), ws
    assert codec.fit_bytes(8, H, W, 5, 3, 64, 2, bs, 10, FeatCfg()) > ws


def test_wide_shape_steps_in_groups():
    assert ops.train_group_size(8, 256, 256, 5, 3, FeatCfg(), 64, 2) == ops.train_group_max() >= 2
    assert ops.train_group_size(8, 256, 256, 5, 3, FeatCfg(activation="relu"), 64, 2) >= 2
    # out of scope: one or three hidden layers at this width, bc = 128 -- nothing fused groups them
    assert ops.train_group_size(8, 256, 256, 5, 3, FeatCfg(), 64, 3) == 1
    assert ops.train_group_size(8, 256, 256, 5, 3, FeatCfg(), 64, 1) == 1
