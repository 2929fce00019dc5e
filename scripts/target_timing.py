"""What `encode.py --target-psnr P` costs beside the way to the same answer on the parent commit, and what the flag it rests on
(LBDRN_EVAL_DECODED) costs the calls that do not set it.

On the 8 x 2048^2 synthetic tile, K = 1..8, medians of 6 (3 runs in each of 2 processes, behind one warm-up run; processes of the
two trees alternate):

  (a) encode.main --target-psnr P --target-k 1 8 on this tree, file read to file written; P is the PSNR of the middle candidate of
      the table a first run logs;
  (b) the same answer on the parent: encode.main_k_points on the same Ks plus one decode.main -org per point, whose PSNR records
      are what a user would read;
  (c) the flagless evaluation pass (ops.eval_sse, canonical, headline shape, HIP events) and the headline of `python bench.py
      --gpus 1 --steps 12 --warmup 4` on the parent and on this tree; the parent measured twice gives the run-to-run spread.

    python scripts/target_timing.py [--parent DIR] [--out profiles/target_timing.txt] [--small]

--parent: the lbdrn-msic_amd directory of a checkout of the parent commit with its libraries built (`git worktree add`, then
build); without it the parent rows read "not measured"."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH = os.path.join(ROOT, "lbdrn-msic_amd")
REPS = 3
KS = list(range(1, 9))


def candidates(path):
    with open(path) as f:
        return [(int(m.group(1)), float(m.group(2))) for m in re.finditer(r"Candidate K=(\d+): .* psnr=(\S+)", f.read())]


def worker(tree, src, workdir, job):
    """-> one JSON line with the job's times (seconds, or ms for the evaluation pass)"""
    sys.path.insert(0, tree)
    stem = os.path.splitext(os.path.basename(src))[0]
    out = {}
    if job == "target":
        import encode
        root = os.path.join(workdir, f"{os.getpid()}-table")
        assert encode.main(["-i", src, "-o", root, "--target-psnr", "0"]) == 0          # warms the command up, and logs the table
        (sub,) = os.listdir(root)
        table = candidates(os.path.join(root, sub, "encode.txt"))
        shutil.rmtree(root)
        P = sorted(p for _, p in table)[len(table) // 2]
        times = []
        for rep in range(REPS):
            root = os.path.join(workdir, f"{os.getpid()}-target-{rep}")
            t0 = time.perf_counter()
            assert encode.main(["-i", src, "-o", root, "--target-psnr", repr(P)]) == 0
            times.append(time.perf_counter() - t0)
            (sub,) = os.listdir(root)
            chosen = int(re.search(r"_K(\d+)_", sub).group(1))
            shutil.rmtree(root)
        out = {"times": times, "target": P, "chosen": chosen, "table": table}
    elif job == "sweep":
        import decode
        import encode
        times = []
        for rep in range(REPS + 1):
            root = os.path.join(workdir, f"{os.getpid()}-sweep-{rep}")
            t0 = time.perf_counter()
            assert all(v is None for v in encode.main_k_points(["-i", src, "-o", root], KS).values())
            t1 = time.perf_counter()
            for sub in sorted(os.listdir(root)):
                assert decode.main(["-i", os.path.join(root, sub, stem + ".bin"), "-org", src]) == 0
            times.append((time.perf_counter() - t0, t1 - t0))
            shutil.rmtree(root)
        out = {"times": [t for t, _ in times[1:]], "fit_times": [t for _, t in times[1:]]}
    elif job == "eval":
        import numpy as np
        import torch
        from lbdrn_hip import ops
        from lbdrn_hip.features import FeatCfg
        dev = torch.device("cuda:0")
        img = np.load(src)
        C, H, W = img.shape
        img_d = ops.to_device_u16(img, dev)
        msb_d, mx = ops.split_bits(img_d, 5)
        geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, FeatCfg(), dev)
        net = ops.make_net(geom.F, 64, C, 2, FeatCfg().act)
        torch.manual_seed(1)
        p = (torch.rand(ops.param_count(net), device=dev) - 0.5) * 0.05
        ws = ops.ApplyWorkspace(geom, net, dev)
        sse = torch.zeros(1, dtype=torch.float64, device=dev)
        for _ in range(3):
            ops.eval_sse(geom, net, img_d, msb_d, p, ws=ws, out=sse)
        times = []
        for _ in range(2 * REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                ops.eval_sse(geom, net, img_d, msb_d, p, ws=ws, out=sse)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / 5)
        out = {"times": times, "sse": float(sse.item())}
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(tree, src, workdir, job):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, src, workdir, job],
                         capture_output=True, text=True, timeout=500)
    if res.returncode != 0:
        raise SystemExit(f"worker {job} for {tree} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    (line,) = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(line[7:])


def run_bench(tree):
    """the headline of bench.py in the checkout that holds `tree` -> Mpixels/s"""
    res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "12", "--warmup", "4"], cwd=os.path.dirname(tree),
                         capture_output=True, text=True, timeout=500)
    if res.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    line = [l for l in res.stdout.splitlines() if l.startswith("{") and '"value"' in l][-1]
    return float(json.loads(line)["value"])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_timing.txt"))
    p.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    p.add_argument("--small", action="store_true", help="a tiny raster and no bench.py: a rehearsal of the script, not a measurement")
    p.add_argument("--part", choices=("all", "encode", "flagless"), default="all", help="(a) and (b), or (c), alone")
    args = p.parse_args()
    if args.worker:
        return worker(*args.worker)
    import numpy as np
    sys.path.insert(0, BRANCH)
    from lbdrn_hip.synth import synthetic_tile
    side = 2048 if not args.small else 160
    got = {}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "tile.npy")
        np.save(src, synthetic_tile(0, 8, side, side))
        for rnd in range(2):                                        # parent and branch alternate
            for who, tree in ([("parent", args.parent)] if args.parent else []) + [("branch", BRANCH)]:
                jobs = (["sweep"] + (["target"] if who == "branch" else []) if args.part != "flagless" else []) + \
                       (["eval"] if args.part != "encode" else [])
                for job in jobs:
                    rec = run_worker(tree, src, d, job)
                    have = got.setdefault((who, job), dict(rec, times=[]))
                    have["times"] += rec["times"]
                    if job == "sweep":
                        have.setdefault("fits", []).extend(rec["fit_times"])
                if args.part != "encode" and not args.small:
                    got.setdefault((who, "bench"), []).append(run_bench(tree))
    med = lambda t: statistics.median(t)
    ms = lambda t, k=1e3: f"{k * med(t):9.1f} ({k * min(t):.1f} .. {k * max(t):.1f})"
    lines = [f"8 x {side} x {side} synthetic tile, -sr 1, K = 1..8, D2 bc64 nl2 e10 bs8192, LBB2; ms, median (min .. max) of {2 * REPS} runs in 2 processes"]
    t = got.get(("branch", "target"))
    if t:
        lines.append(f"  (a) branch  encode.main --target-psnr {t['target']!r} --target-k 1 8 (chose K={t['chosen']}): {ms(t['times'])}")
        lines.append("      the table: " + "  ".join(f"K={k}: {v:.2f} dB" for k, v in t["table"]))
    for who in ("parent", "branch"):
        s = got.get((who, "sweep"))
        lines.append(f"  (b) {who:6s}  main_k_points(K = 1..8) + 8 x decode.main -org: " +
                     (f"{ms(s['times'])}, of which main_k_points {ms(s['fits'])}" if s else "not measured"))
    if t and got.get(("parent", "sweep")):
        lines.append(f"      (a) / (b on the parent) = {med(t['times']) / med(got[('parent', 'sweep')]['times']):.3f}")
    for who in ("parent", "branch"):
        e, b = got.get((who, "eval")), got.get((who, "bench"))
        lines.append(f"  (c) {who:6s}  flagless lbdrn_eval_sse, canonical, K5: " + (f"{ms(e['times'], 1.0)} ms (sum {e['sse']!r})" if e else "not measured") +
                     "; bench.py --gpus 1 --steps 12 --warmup 4: " + (" and ".join(f"{v:.2f}" for v in b) + " Mpixels/s" if b else "not measured"))
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
