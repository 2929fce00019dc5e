"""Generate tests/golden/d3_bands8.npz by RUNNING the reference's own modules (authoring container only; needs the
reference checkout MG.REF points at).  Modelled on make_golden_bands4.py.

The reference's D = 3 sweep (run.sh: `./run.sh 3 3 64 2 0.001 8192 10 1 outputs-rel-colors-D3`) on its 8-band images:
F = 8 * 7 * 7 = 392 features, 384 that can differ from zero (the window centres are exact zeros, LBDRNdataset.py:126-128)
-- the shape of the wide fused training step (k_train_split at LQ = 96).

d3_bands8.npz
  params0    the reference LBDRNModel(392, 64, 8, 2) under seed 19920517: the initial parameters of every case below;
  small/*    an 8 x 24 x 20 image and its labels from the reference's LBDRNdataset.process() (C = 8, D = 3, relative colours;
             the 480 x 392 feature matrix is not stored -- 1 MiB of file budget -- the oracle builds it, and
             test_gpu_wide_window checks the first step's gradient, which depends on every feature), six teacher-forced
             updates of 96-row minibatches with the reference's LBDRNLoss, torch.optim.Adam and StepLR as encode.py:84-86
             builds them (modified_ignite_engine.py:18-27 replayed): the gradient of the first step, loss and learning rate
             of every step, the parameters after the first and the last step, the Adam moments at the end;
  ragged/*   an 8 x 40 x 52 image (2080 rows), six teacher-forced updates of 200-row minibatches (three whole 64-row groups
             and one of eight rows: the last 32-row workgroups partly filled or empty): losses, parameters after the last step;
  relu/*     the `small` image and minibatches with activation=torch.nn.ReLU() (encode.py:75's alternative), likewise.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_round3 as R3  # noqa: E402  (process())

SEED = MG.SEED


def teacher_forced(LBDRNModel, loss_fn, f, l, C, rows, gseed, out, tag, full, **kw):
    F = f.shape[1]
    torch.manual_seed(SEED)
    m = LBDRNModel(dim_in=F, dim_hidden=64, dim_out=C, num_layers=2, **kw)      # encode.py:71-77
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)                               # encode.py:84
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=max(1, int(3 / 3)), gamma=0.1)
    g = torch.Generator().manual_seed(gseed)
    p0 = MG._flat(m.state_dict())
    if "params0" in out:
        assert np.array_equal(out["params0"], p0)   # (one initialisation for all three: same seed, same shape)
    out["params0"] = p0
    nsteps = 6
    batches = np.stack([torch.randperm(f.shape[0], generator=g)[:rows].numpy() for _ in range(nsteps)])
    out[tag + "/batches"] = batches.astype(np.int64)
    losses, lrs = [], []
    for s in range(nsteps):
        x, t = torch.from_numpy(f[batches[s]]), torch.from_numpy(l[batches[s]])
        opt.zero_grad()
        m.train()
        loss = loss_fn(m(x), t)                                                   # modified_ignite_engine.py:18-27
        loss.backward()
        if full and s == 0:
            out[tag + "/step0/grads"] = np.concatenate([p.grad.numpy().reshape(-1) for p in m.parameters()])
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        losses.append(loss.item())
        if s == nsteps - 1 or (full and s == 0):
            out[f"{tag}/step{s}/params"] = MG._flat(m.state_dict())
        if s % 2 == 1:
            sched.step()   # an "epoch" of two iterations: encode.py:98
    out[tag + "/losses"] = np.array(losses, np.float32)
    out[tag + "/lrs"] = np.array(lrs, np.float64)
    if full:
        out[tag + "/exp_avg"] = np.concatenate([opt.state[p]["exp_avg"].numpy().reshape(-1) for p in m.parameters()])
        out[tag + "/exp_avg_sq"] = np.concatenate([opt.state[p]["exp_avg_sq"].numpy().reshape(-1) for p in m.parameters()])


def main():
    sys.path.insert(0, MG.REF)
    MG._install_standins()
    import LBDRNdataset as RD
    from LBDRNloss import LBDRNLoss
    from LBDRNmodel import LBDRNModel
    loss_fn = LBDRNLoss()
    K, D, C = 5, 3, 8
    out = {}

    img = MG._img(51, C, 24, 20)
    f, l = R3.process(RD, img, K, D, {})
    assert f.shape == (480, 392) and l.shape == (480, C)
    out["small/img"] = img
    out["small/labels"] = l
    teacher_forced(LBDRNModel, loss_fn, f, l, C, 96, 53, out, "small", True)
    teacher_forced(LBDRNModel, loss_fn, f, l, C, 96, 53, out, "relu", False, activation=torch.nn.ReLU())

    img2 = MG._img(52, C, 40, 52)
    f2, l2 = R3.process(RD, img2, K, D, {})
    out["ragged/img"] = img2
    teacher_forced(LBDRNModel, loss_fn, f2, l2, C, 200, 54, out, "ragged", False)
    path = os.path.join(HERE, "d3_bands8.npz")
    np.savez_compressed(path, **out)
    print("d3_bands8.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
