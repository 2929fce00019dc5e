"""The wide fused training step (k_train_split<96, 24>: bc = 64, nl = 2, D = 3 on 8 bands, 384 features multiplied) against
the generic kernels (LBDRN_PATH_GENERIC) on one 8 x 2048 x 2048 tile at D3 K5 bc64 nl2 bs 8192:
  * ms per training epoch (lbdrn_train_epoch alone, no evaluation pass), fused for a lone fit (LBDRN_TRAIN_ALONE) and without
    the hint, generic;
  * ms per tile of whole fits (fit_many: 10 epochs with their evaluation passes), one fit alone and four in flight, fused
    (PATH_AUTO) and generic.
usage: wide_window_timing.py [epochs=10] [--kernel-only]   (--kernel-only: lone fused epochs only, for a rocprofv3 run)

The step executes 126 k MFMA FLOP per row (2 x 64 x 384 for layer 0 forward and again for dW_0, 2 x 64 x 64 for the hidden
layer's forward, backward and dW_1, 2 x 16 x 64 for the output layer's forward, backward and dW_last on 16 channel slots).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lbdrn_hip import codec, ops  # noqa: E402
from lbdrn_hip.features import FeatCfg  # noqa: E402
from lbdrn_hip.synth import synthetic_tile  # noqa: E402

FLOP_PER_ROW = 2 * 64 * 384 * 2 + 2 * 64 * 64 * 3 + 2 * 16 * 64 * 3
args = [a for a in sys.argv[1:] if not a.startswith("--")]
epochs = int(args[0]) if args else 10
kernel_only = "--kernel-only" in sys.argv
dev = torch.device("cuda:0")
K, D, bc, nl, bs, side = 5, 3, 64, 2, 8192, 2048
cfg = FeatCfg()
img = ops.to_device_u16(synthetic_tile(1000, 8, side, side), dev)
msb, mx = ops.split_bits(img, K)
geom = ops.FeatureGeometry(8, side, side, K, D, mx, cfg, dev)
net = ops.make_net(cfg.feature_dim(8, D), bc, 8, nl, cfg.act)
N = side * side
steps = (N + bs - 1) // bs
print(f"shape: 8 x {side}^2, D{D} K{K} bc{bc} nl{nl} bs{bs}: F = {net.F}, step features {ops.train_step_features(geom, net)}, "
      f"{FLOP_PER_ROW} MFMA FLOP per row, {steps} steps per epoch", flush=True)


def epochs_ms(path, alone, n):
    torch.manual_seed(1)
    p = torch.from_numpy(np.random.default_rng(1).uniform(-1e-3, 1e-3, ops.param_count(net)).astype(np.float32)).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img, msb, path)
    perm = torch.randperm(N, device=dev)
    ops.train_epoch(geom, net, img, msb, perm, bs, p, m, v, 0, 1e-3, losses, path, ws, alone=alone)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e in range(n):
        ops.train_epoch(geom, net, img, msb, perm, bs, p, m, v, (e + 1) * steps, 1e-3, losses, path, ws, alone=alone)
    torch.cuda.synchronize()
    del ws
    return 1e3 * (time.perf_counter() - t0) / n


if kernel_only:
    print(f"fused, lone fit: {epochs_ms(ops._lib.PATH_MFMA, True, epochs):.2f} ms per epoch", flush=True)
    sys.exit(0)
res = {}
for name, path, alone in (("fused, lone fit", ops._lib.PATH_MFMA, True), ("fused, no hint", ops._lib.PATH_MFMA, False),
                          ("generic", ops._lib.PATH_GENERIC, True)):
    res[name] = epochs_ms(path, alone, epochs if path != ops._lib.PATH_GENERIC else 2)
    print(f"train epoch {name:16s}: {res[name]:8.2f} ms ({res[name] * 1e3 / steps:6.1f} us a step)", flush=True)
print(f"lone fused epoch vs generic: {res['generic'] / res['fused, lone fit']:.2f}x faster", flush=True)
torch.cuda.empty_cache()
for path, pname in ((ops.PATH_AUTO, "fused (auto)"), (ops._lib.PATH_GENERIC, "generic")):
    for n in (1, 4):
        imgs = [ops.to_device_u16(synthetic_tile(2000 + k, 8, side, side), dev) for k in range(n)]
        codec.fit_many(imgs[:1], K, D, bc, nl, 1e-3, bs, 1, cfg=cfg, path=path, in_flight=1)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codec.fit_many(imgs, K, D, bc, nl, 1e-3, bs, epochs, cfg=cfg, path=path, in_flight=n)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"fit_many {pname:12s}, {n} in flight, {epochs} epochs: {ms:9.1f} ms = {ms / n:8.1f} ms per tile", flush=True)
        del imgs
        torch.cuda.empty_cache()
