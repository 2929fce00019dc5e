"""What a K sweep of one image costs with its K points fitted side by side (`sweep.py --k-in-flight 6`) against point
after point (`--k-in-flight 1`, the default) and against the parent commit's sweep.py.

K = 1 .. 6 at -sr 1 (the reference's run.sh protocol) on the synthetic 8 x 2048^2 tile and on a 4 x 2048^2 one; every
other setting is sweep.py's default (bc 64, nl 2, D 2, 10 epochs, minibatches of 8192 rows, LBB2 payloads).  One run is one
fresh process: a warm-up sweep of K = 1 alone into a directory of its own (library load, allocator, first launches),
then the counted sweep -- wall time of sweep.main(), encode and decode of all six points, and the `fit ...s on` record of
every point's encode.txt.  Three counted runs per arm, the arms alternating.  Also: how many fits
codec.memory_limited_in_flight lets progress together at the two reference scene sizes (8 x 6000^2, 4 x 7550^2) when the six
K points of ONE scene are handed over, against six different scenes, with this device's free memory.

    python scripts/sweep_in_flight_timing.py [--parent DIR] [--out profiles/sweep_in_flight_timing.txt] [--small]

--parent: the lbdrn-msic_amd directory of a checkout of the parent commit with its libraries built; without it the parent
arm reads "not measured".  --small: tiny rasters and two epochs, a rehearsal of the script, writes nothing."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH = os.path.join(ROOT, "lbdrn-msic_amd")
RUNS = 3
K_RANGE = (1, 6)


def worker(tree, image, out_dir, extra):
    """One process: warm-up sweep (K = 1), counted sweep -> one JSON line {wall, fit: [seconds per point]}."""
    sys.path.insert(0, tree)
    os.chdir(tree)
    import sweep
    assert sweep.main(["--images", image, "--k", "1", "1", "-o", os.path.join(out_dir, "warm")] + extra) == 0
    counted = os.path.join(out_dir, "counted")
    t0 = time.perf_counter()
    assert sweep.main(["--images", image, "--k", str(K_RANGE[0]), str(K_RANGE[1]), "-o", counted] + extra) == 0
    wall = time.perf_counter() - t0
    fit = []
    for sub in sorted(os.listdir(counted)):
        with open(os.path.join(counted, sub, "encode.txt")) as f:
            fit += [float(x) for x in re.findall(r": fit ([0-9.]+)s on ", f.read())]
    assert len(fit) == K_RANGE[1] - K_RANGE[0] + 1, fit
    print("RESULT " + json.dumps({"wall": wall, "fit": fit}), flush=True)


def run_worker(tree, image, out_dir, extra):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, image, out_dir, json.dumps(extra)],
                         capture_output=True, text=True, timeout=400)
    if res.returncode != 0:
        raise SystemExit(f"worker for {tree} {extra} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    (line,) = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(line[7:])


def limiter_lines():
    import torch
    from lbdrn_hip import codec

    class Scene:
        def __init__(self, ptr, *shape):
            self.ptr, self.shape, self.device = ptr, shape, torch.device("cuda:0")

        def data_ptr(self):
            return self.ptr
    free, total = torch.cuda.mem_get_info(torch.device("cuda:0"))
    lines = [f"codec.memory_limited_in_flight, six fits wanted, K = 1 .. 6, D 2 bc 64 nl 2, 10 epochs, minibatches of 8192 rows; "
             f"{free / 2**30:.0f} GiB free of {total / 2**30:.0f}"]
    Ks = list(range(1, 7))
    for C, side in ((8, 6000), (4, 7550)):
        one = codec.memory_limited_in_flight([Scene(1, C, side, side)] * 6, 6, Ks, 2, 64, 2, 8192, 10)
        six = codec.memory_limited_in_flight([Scene(k, C, side, side) for k in range(6)], 6, Ks, 2, 64, 2, 8192, 10)
        need = codec.fit_bytes(C, side, side, Ks, 2, 64, 2, 8192, 10)
        lines.append(f"  {C} x {side}^2: one fit {need / 2**30:.1f} GiB of which the scene {codec.image_bytes(C, side, side) / 2**30:.2f}; "
                     f"fits allowed in flight: {one} (the six K points of one scene), {six} (six scenes)")
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_in_flight_timing.txt"))
    p.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    p.add_argument("--small", action="store_true", help="tiny rasters: a rehearsal of the script, not a measurement")
    args = p.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.worker[2], json.loads(args.worker[3]))
    sys.path.insert(0, BRANCH)
    import numpy as np
    from lbdrn_hip.synth import synthetic_tile
    side = 2048 if not args.small else 64
    common = [] if not args.small else ["-e", "2", "-bs", "512"]
    arms = [("parent", args.parent, []), ("--k-in-flight 1", BRANCH, ["--k-in-flight", "1"]),
            ("--k-in-flight 6", BRANCH, ["--k-in-flight", "6"])]
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for C in (8, 4):
            image = os.path.join(d, f"tile{C}.npy")
            np.save(image, synthetic_tile(0, C, side, side))
            got = {}
            for run in range(RUNS):                                     # the arms alternate
                for name, tree, extra in arms:
                    if tree is not None:
                        res = run_worker(os.path.abspath(tree), image, os.path.join(d, f"{C}-{name}-{run}"), common + extra)
                        print(f"{C} bands, run {run}, {name}: {res['wall']:.2f} s", flush=True)
                        got.setdefault(name, []).append(res)
            lines.append(f"{C} x {side} x {side}, sweep.py --k 1 6 -sr 1 (bc64 nl2 D2, LBB2): {RUNS} counted runs per arm, one process each, "
                         f"the arms alternating")
            lines.append("  arm                wall s per sweep: median (min .. max)    fit ms per point, from the `fit` records: "
                         "median of the runs' means (min .. max)")
            for name, tree, _ in arms:
                if tree is None:
                    lines.append(f"  {name:17s}  not measured")
                    continue
                wall = [r["wall"] for r in got[name]]
                fit = [1e3 * statistics.mean(r["fit"]) for r in got[name]]
                lines.append(f"  {name:17s}  {statistics.median(wall):7.2f} ({min(wall):.2f} .. {max(wall):.2f})"
                             f"                   {statistics.median(fit):7.1f} ({min(fit):.1f} .. {max(fit):.1f})")
    lines += limiter_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
