"""The fused apply pass's kernels alone on one 2048 x 2048 tile of BANDS bands (bc = 64, nl = 2, D = 2, K = 5): twenty fast evaluation
passes (k_apply_mfma<2,2,false>), twenty decode passes (<2,0,false>) and five canonical evaluation passes (<2,1,false>), each
kind timed by a host clock around a synchronise.  Meant to run under `rocprofv3 --kernel-trace --stats` once per library
(LBDRN_HIP_LIB) and band count, the libraries alternating: DESIGN.md 4.6.

    python scripts/apply_blocks4_timing.py BANDS"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lbdrn-msic_amd"))
import torch  # noqa: E402

from lbdrn_hip import ops  # noqa: E402
from lbdrn_hip.features import FeatCfg  # noqa: E402
from lbdrn_hip.synth import synthetic_tile  # noqa: E402

bands = int(sys.argv[1]) if len(sys.argv) > 1 else 8
dev = torch.device("cuda:0")
img_d = ops.to_device_u16(synthetic_tile(0, bands, 2048, 2048), dev)
msb_d, mx = ops.split_bits(img_d, 5)
cfg = FeatCfg()
geom = ops.FeatureGeometry(bands, 2048, 2048, 5, 2, mx, cfg, dev)
net = ops.make_net(cfg.feature_dim(bands, 2), 64, bands, 2)
torch.manual_seed(0)
p = (torch.rand(ops.param_count(net), device=dev) - 0.5) * 0.05
ws = ops.ApplyWorkspace(geom, net, dev)


def timed(name, n, call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        r = call()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / n
    tail = f"  sse={float(r.item()):.9f}" if r.numel() == 1 else ""
    print(f"bands={bands} {name}: {dt * 1e3:.3f} ms per pass{tail}")


timed("fast evaluation", 20, lambda: ops.eval_sse(geom, net, img_d, msb_d, p, ws=ws, fast=True))
timed("decode", 20, lambda: ops.decode_fused(geom, net, msb_d, p, ws=ws))
timed("canonical evaluation", 5, lambda: ops.eval_sse(geom, net, img_d, msb_d, p, ws=ws))
