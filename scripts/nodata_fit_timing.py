"""What `encode.py --nodata V --nodata-fit valid` buys in time and does to quality on one full-size tile, beside `--nodata V`
alone on this commit and on the parent commit.

The tile is scripts/nodata_timing.py's: the 8 x 2048^2 synthetic one with 0 outside the largest square that fits the frame when
turned by 12 degrees.  Every measurement is the wall time of encode.main() / decode.main(), file read to file written, in a
process that has run the same command once before; processes of the two trees alternate.  Beside the times: the `Nodata fit:`
record (the steps per epoch), the file size, and the `MSE:` / `PSNR:` records of one `decode.py -org` run of each file -- nodata
samples decode exactly either way, so the all-sample MSE compares the valid samples directly.

    python scripts/nodata_fit_timing.py [--parent DIR] [--out profiles/nodata_fit_timing.txt] [--small]

--parent: the lbdrn-msic_amd directory of a checkout of the parent commit with its libraries built (`git worktree add`, then
build); without it the parent row reads "not measured"."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH = os.path.join(ROOT, "lbdrn-msic_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nodata_timing import collared_tile  # noqa: E402

REPS = 3
JOBS = {"nodata": ["--nodata", "0"], "nodata-fit valid": ["--nodata", "0", "--nodata-fit", "valid"]}


def records(path, heads):
    got = {}
    with open(path) as f:
        for line in f:
            text = line.split("] ", 1)[-1].strip()
            for h in heads:
                if text.startswith(h):
                    got[h] = text[len(h):].strip()
    return got


def worker(tree, src, workdir, labels):
    """-> one JSON line {label: {"encode": [s, ...], "decode": [s, ...], "bytes": n, "fit": record or None, "mse": .., "psnr": ..}}"""
    sys.path.insert(0, tree)
    import decode
    import encode
    out = {}
    for label in labels:
        enc, dec = [], []
        for rep in range(REPS + 1):                       # the first run warms the command up
            root = os.path.join(workdir, f"{os.getpid()}-{label.replace(' ', '_')}-{rep}")
            t0 = time.perf_counter()
            assert encode.main(["-i", src, "-o", root] + JOBS[label]) == 0
            enc.append(time.perf_counter() - t0)
            (sub,) = os.listdir(root)
            binp = os.path.join(root, sub, os.path.splitext(os.path.basename(src))[0] + ".bin")
            t0 = time.perf_counter()
            assert decode.main(["-i", binp]) == 0
            dec.append(time.perf_counter() - t0)
            size = os.path.getsize(binp)
            if rep == REPS:                               # quality, once, outside the timed calls
                fit = records(os.path.join(root, sub, "encode.txt"), ["Nodata fit:"]).get("Nodata fit:")
                os.remove(os.path.join(root, sub, "decode.txt"))
                assert decode.main(["-i", binp, "-org", src]) == 0
                q = records(os.path.join(root, sub, "decode.txt"), ["MSE:", "PSNR:"])
            shutil.rmtree(root)                           # (a .bin and a 64 MB raster per run)
        out[label] = {"encode": enc[1:], "decode": dec[1:], "bytes": size, "fit": fit, "mse": q.get("MSE:"), "psnr": q.get("PSNR:")}
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(tree, src, workdir, labels):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, src, workdir, json.dumps(labels)],
                         capture_output=True, text=True, timeout=500)
    if res.returncode != 0:
        raise SystemExit(f"worker for {tree} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    (line,) = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(line[7:])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodata_fit_timing.txt"))
    p.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    p.add_argument("--small", action="store_true", help="a tiny raster: a rehearsal of the script, not a measurement")
    args = p.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.worker[2], json.loads(args.worker[3]))
    import numpy as np
    side = 2048 if not args.small else 160
    got = {}
    with tempfile.TemporaryDirectory() as d:
        img, share = collared_tile(side)
        src = os.path.join(d, "tile.npy")
        np.save(src, img)
        for rnd in range(2):                                        # parent and branch alternate
            trees = ([("parent", args.parent, ["nodata"])] if args.parent else []) + [("branch", BRANCH, list(JOBS))]
            for who, tree, labels in trees:
                for label, rec in run_worker(tree, src, d, labels).items():
                    have = got.setdefault((who, label), dict(rec, encode=[], decode=[]))
                    have["encode"] += rec["encode"]
                    have["decode"] += rec["decode"]
                    assert all(have[k] == rec[k] for k in ("bytes", "fit", "mse", "psnr")), (have, rec)
    ms = lambda t: f"{1e3 * statistics.median(t):8.1f} ({1e3 * min(t):.1f} .. {1e3 * max(t):.1f})"
    lines = [f"8 x {side} x {side} synthetic tile, collar of {100 * share:.1f} % set to 0, --nodata 0, -sr 1, K5 D2 bc64 nl2 e10 bs8192, LBB2; "
             f"wall time of encode.main / decode.main, ms, median (min .. max) of {2 * REPS} runs in 2 processes; sizes in bytes; MSE / PSNR: the "
             "records of decode.py -org (all samples; nodata samples decode exactly in every row)",
             f"  {'':6s} {'':18s} {'encode.main':>30s} {'decode.main':>30s} {'file':>12s} {'MSE':>22s} {'PSNR':>20s}  fit"]
    for who in ("parent", "branch"):
        for label in JOBS:
            rec = got.get((who, label))
            if rec is None:
                if who == "parent" and label == "nodata":
                    lines.append(f"  {who:6s} {label:18s} not measured")
                continue
            lines.append(f"  {who:6s} {label:18s} {ms(rec['encode']):>30s} {ms(rec['decode']):>30s} {rec['bytes']:12d} {rec['mse']:>22s} "
                         f"{rec['psnr']:>20s}  {rec['fit'] or f'{side * side} of {side * side} pixels, {-(-side * side // 8192)} steps per epoch'}")
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
