"""fit_many of four 8 x 2048^2 tiles, two pairs in flight: fits that seed themselves alike -- codec.fit_group gives the fits
of a pair ONE permutation stream, each epoch's permutation is generated once -- against fits that bring different draws
(one stream per fit).  Six alternating repetitions in one process, ms per tile.  -> profiles/sweep_in_flight_timing.txt"""
import os, sys, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))
import torch
from lbdrn_hip import codec, ops
from lbdrn_hip.features import FeatCfg
from lbdrn_hip.synth import synthetic_tile
dev = torch.device("cuda:0")
tiles = [ops.to_device_u16(synthetic_tile(k, 8, 2048, 2048), dev) for k in range(4)]
cfg = FeatCfg()
def run(kind):
    if kind == "same":
        kw = dict(seed=19920517)
    else:
        torch.manual_seed(1)
        kw = dict(draws=[codec.draw_fit(200, 64, 8, 2, 10) for _ in range(4)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codec.fit_many(tiles, 5, 2, 64, 2, 1e-3, 8192, 10, cfg=cfg, in_flight=4, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / 4
for kind in ("same", "different"):
    run(kind)
got = {"same": [], "different": []}
for rep in range(6):
    for kind in got:
        got[kind].append(run(kind))
for kind, t in got.items():
    print(f"{kind}: ms per tile median {statistics.median(t):.2f} ({min(t):.2f} .. {max(t):.2f})", flush=True)
