"""The autograd entry points' host side: sizes without a device, the no-device answer, and the split of the flat
gradient vector into per-parameter views (lbdrn_hip.autograd)."""
import ctypes

import pytest
import torch
from torch import nn


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("F,bc,C,nl,B", [(200, 64, 8, 2, 8192), (18, 16, 3, 3, 64), (27, 32, 3, 1, 1000),
                                         (200, 256, 8, 2, 257), (250, 64, 8, 2, 1), (100, 64, 4, 2, 0)])
def test_tape_and_workspace_sizes_without_device(F, bc, C, nl, B):
    from lbdrn_hip import _lib
    L = _lib.lib()
    net = _lib.Net(F, bc, C, nl, 0)
    half = _align(nl * B * bc * 4)
    assert L.lbdrn_tape_bytes(ctypes.byref(net), B) == 2 * half
    slices = (B + 255) // 256
    want = _align(B * C * 4) + 2 * _align(B * bc * 4) + _align(slices * max(bc, C) * (max(bc, F) + 1) * 4)
    assert L.lbdrn_backward_workspace(ctypes.byref(net), B) == want
    # the activation does not change the sizes; a bad net or a negative batch sizes to 0
    assert L.lbdrn_tape_bytes(ctypes.byref(_lib.Net(F, bc, C, nl, 1)), B) == 2 * half
    assert L.lbdrn_tape_bytes(ctypes.byref(_lib.Net(F, bc, C, 0, 0)), B) == 0
    assert L.lbdrn_backward_workspace(ctypes.byref(net), -1) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_backward_without_device_says_so():
    from lbdrn_hip import _lib
    L = _lib.lib()
    net = _lib.Net(200, 64, 8, 2, 0)
    fake = ctypes.c_void_p(256)        # never dereferenced: the device check comes first
    # argument checks come before the device check, as in lbdrn_forward
    assert L.lbdrn_backward(ctypes.byref(net), fake, fake, 16, fake, 1 << 20, fake, None, fake, None, fake, 1 << 20,
                            None) == _lib.E_ARG
    assert b"null" in L.lbdrn_last_error()
    rc = L.lbdrn_backward(ctypes.byref(net), fake, fake, 16, fake, 1 << 20, fake, fake, fake, None, fake, 1 << 20, None)
    assert rc == _lib.E_DEVICE
    assert b"no CPU path" in L.lbdrn_last_error() or b"HIP" in L.lbdrn_last_error()
    assert L.lbdrn_forward_tape(ctypes.byref(net), fake, fake, 16, fake, fake, 1 << 20, None) == _lib.E_DEVICE
    assert b"no CPU path" in L.lbdrn_last_error() or b"HIP" in L.lbdrn_last_error()


@pytest.mark.parametrize("nl", (1, 2, 3))
@pytest.mark.parametrize("relu", (False, True))
def test_flat_gradient_splits_into_state_dict_views(nl, relu):
    from lbdrn_hip import _lib, autograd
    from lbdrn_hip.model import LBDRNModel
    torch.manual_seed(nl)
    m = LBDRNModel(27, 16, 3, nl, activation=nn.ReLU() if relu else None)
    sd = m.state_dict()
    params = m.hip_parameters()
    assert [p.shape for p in params] == [v.shape for v in sd.values()]
    assert all(isinstance(p, nn.Parameter) for p in params)
    assert [id(p) for p in params] == [id(dict(m.named_parameters())[k]) for k in sd]
    flat = m.flat_parameters()
    assert flat.numel() == _lib.lib().lbdrn_param_count(ctypes.byref(m.hip_net()))
    views = autograd.split_flat(flat, [p.shape for p in params])
    assert len(views) == len(sd)
    for v, (k, ref) in zip(views, sd.items()):
        assert v.shape == ref.shape and torch.equal(v, ref), k
        assert v.data_ptr() >= flat.data_ptr() and v.data_ptr() < flat.data_ptr() + flat.numel() * 4   # views, no copy
    with pytest.raises(ValueError):
        autograd.split_flat(flat[:-1], [p.shape for p in params])


def test_output_records_no_graph_unless_explicitly_training():
    """Host side of the recording rule: eval() clears what train() set; a fresh module has it cleared."""
    from lbdrn_hip.model import LBDRNModel
    m = LBDRNModel(8, 16, 2, 1)
    assert m.training and not m._explicit_train
    m.train()
    assert m._explicit_train
    m.eval()
    assert not m.training and not m._explicit_train
    m.train(False)
    assert not m._explicit_train
