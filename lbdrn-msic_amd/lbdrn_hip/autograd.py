"""torch.autograd for LBDRNModel: the forward keeps a tape in liblbdrn_hip (lbdrn_forward_tape), the backward turns
torch's dL/dy into parameter gradients and dL/dx there (lbdrn_backward).  What `loss.backward()` does on the
reference's model (ref modified_ignite_engine.py:24, the autograd of LBDRNmodel.py:39-43,79-82); torch accumulates the
returned gradients into `.grad`, the optimiser and the loss stay torch's."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops


def split_flat(flat, shapes):
    """Views of the flat state_dict-order vector `flat`, one per shape of `shapes` (in that order)."""
    sizes = [torch.Size(s).numel() for s in shapes]
    if sum(sizes) != flat.numel():
        raise ValueError(f"flat vector of {flat.numel()} values for parameters of {sum(sizes)}")
    out, o = [], 0
    for shape, n in zip(shapes, sizes):
        out.append(flat[o:o + n].view(shape))
        o += n
    return out


class LBDRNFunction(torch.autograd.Function):
    """apply(net, x, *params): params are the module's parameters in state_dict order, on x's device."""

    @staticmethod
    def forward(ctx, net, x, *params):
        for p in params:
            if p.device != x.device:
                raise _lib.LbdrnError(f"LBDRNModel parameters are on {p.device} but x is on {x.device}: move the model "
                                      "with model.to(x.device) first (autograd does not copy them)")
        flat = torch.cat([p.reshape(-1) for p in params])
        y, tape = ops.forward_tape(net, flat, x)
        ctx.net = net
        ctx.shapes = [p.shape for p in params]
        ctx.save_for_backward(x, y, tape, flat)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, tape, flat = ctx.saved_tensors
        want_dx = ctx.needs_input_grad[1]
        grads, dx = ops.backward(ctx.net, flat, x, tape, y, dy, want_dx=want_dx)
        views = split_flat(grads, ctx.shapes)
        return (None, dx, *[g if need else None for g, need in zip(views, ctx.needs_input_grad[2:])])
