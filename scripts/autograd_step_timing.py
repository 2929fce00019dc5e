"""One training step through torch autograd against the generic fused-loss step, at the headline shape.

    python scripts/autograd_step_timing.py [--steps 50] [--warmup 10] [--B 8192]

The autograd step is the reference's `_update` (modified_ignite_engine.py:18-27): zero_grad, train(), forward on the
drop-in LBDRNModel (lbdrn_forward_tape), LBDRNLoss (torch's mse_loss), backward (torch's MSE backward, then
lbdrn_backward), torch.optim.Adam.step.  The comparison is ops.train_step (lbdrn_train_step: the same generic kernels
with the loss and Adam fused in).  Both on one fixed minibatch, timed with one HIP-event pair around `--steps` steps.
Prints one JSON line.  To split the library's kernels from torch's, run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python scripts/autograd_step_timing.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lbdrn-msic_amd"))
from lbdrn_hip import ops  # noqa: E402
from lbdrn_hip.model import LBDRNLoss, LBDRNModel  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    a = ap.parse_args()
    F, bc, C, nl, B, lr = 200, 64, 8, 2, a.B, 1e-3
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = LBDRNModel(F, bc, C, nl).to(dev)
    p0 = model.flat_parameters().to(dev)
    x = torch.rand(B, F, device=dev) * 2 - 1
    t = torch.randint(0, 32, (B, C), device=dev).float() / 31
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    loss_fn = LBDRNLoss()

    def autograd_step():
        optimizer.zero_grad()
        model.train()
        y_pred = model(x)
        loss = loss_fn(y_pred, t)
        loss.backward()
        optimizer.step()

    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    state = {"step": 0}

    def fused_loss_step():
        state["step"] += 1
        ops.train_step(ops.make_net(F, bc, C, nl), x, t, p, m, v, state["step"], lr)

    ms_autograd = timed(autograd_step, a.steps, a.warmup)
    ms_generic = timed(fused_loss_step, a.steps, a.warmup)
    print(json.dumps({"shape": {"F": F, "bc": bc, "C": C, "nl": nl, "B": B}, "steps": a.steps,
                      "autograd_step_ms": round(ms_autograd, 4), "generic_train_step_ms": round(ms_generic, 4),
                      "ratio": round(ms_autograd / ms_generic, 3)}))


if __name__ == "__main__":
    main()
