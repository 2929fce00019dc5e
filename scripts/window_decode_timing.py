"""What `decode.py --window` costs beside the whole decode of the same file, and whether the whole decode costs what it
did on the parent commit.

Two files, one epoch each (the fit's quality does not matter to the decoder): the 8 x 2048^2 tile at -sr 1, and an
8 x 3072^2 scene at -sr 3 (nine 1024^2 tiles).  The window is 512^2 in the middle of one tile (of the centre tile at -sr 3).
Every measurement is the wall time of decode.main() -- file read to raster written, so it ends after the device has
finished -- in a process that has decoded the same thing once before; processes of the two trees alternate.

    python scripts/window_decode_timing.py [--parent DIR] [--out profiles/window_decode_timing.txt]

--parent: the lbdrn-msic_amd directory of a checkout of the parent commit with its libraries built (`git worktree add`,
then build); without it the parent column reads "not measured"."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH = os.path.join(ROOT, "lbdrn-msic_amd")
REPS = 5


def worker(tree, jobs):
    """jobs: [[label, bin, window or None], ...] -> one JSON line {label: [seconds, ...]}."""
    sys.path.insert(0, tree)
    import decode
    out = {}
    for label, binp, window in jobs:
        argv = ["-i", binp] + (["--window"] + [str(v) for v in window] if window else [])
        times = []
        for rep in range(REPS + 1):                       # the first run warms this shape up
            t0 = time.perf_counter()
            assert decode.main(argv) == 0
            times.append(time.perf_counter() - t0)
        out[label] = times[1:]
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(tree, jobs):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, json.dumps(jobs)],
                         capture_output=True, text=True, timeout=200)
    if res.returncode != 0:
        raise SystemExit(f"worker for {tree} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    (line,) = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(line[7:])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_decode_timing.txt"))
    p.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    p.add_argument("--small", action="store_true", help="tiny rasters: a rehearsal of the script, not a measurement")
    args = p.parse_args()
    if args.worker:
        return worker(args.worker[0], json.loads(args.worker[1]))
    sys.path.insert(0, BRANCH)
    import numpy as np
    import encode
    from lbdrn_hip.synth import synthetic_tile
    side1, side3, win = (2048, 3072, 512) if not args.small else (96, 144, 16)
    lines = []
    with tempfile.TemporaryDirectory() as d:
        files = []
        for name, side, sr in (("tile", side1, 1), ("scene", side3, 3)):
            src = os.path.join(d, name + ".npy")
            np.save(src, synthetic_tile(0, 8, side, side))
            assert encode.main(["-i", src, "-o", os.path.join(d, name), "-e", "1", "-sr", str(sr)]) == 0
            (sub,) = os.listdir(os.path.join(d, name))
            x0 = (side - win) // 2
            files.append((name, side, sr, os.path.join(d, name, sub, name + ".bin"), [x0, x0, win, win]))
        full = [[f"{name} full", binp, None] for name, _, _, binp, _ in files]
        windowed = [[f"{name} window", binp, w] for name, _, _, binp, w in files]
        got = {}
        for rnd in range(2):                                        # parent and branch alternate
            trees = ([("parent", args.parent, full)] if args.parent else []) + [("branch", BRANCH, full + windowed)]
            for who, tree, jobs in trees:
                for label, times in run_worker(tree, jobs).items():
                    got.setdefault((who, label), []).extend(times)
        for name, side, sr, binp, w in files:
            lines.append(f"8 x {side} x {side}, -sr {sr}, K5 D2 bc64 nl2, LBB2, {os.path.getsize(binp)} bytes; window x0={w[0]} y0={w[1]} "
                         f"w={w[2]} h={w[3]}; decode.main wall time, ms, median (min .. max) of {2 * REPS} runs in 2 processes")
            for who, label in (("parent", f"{name} full"), ("branch", f"{name} full"), ("branch", f"{name} window")):
                t = got.get((who, label))
                what = f"{who:6s} {'--window' if label.endswith('window') else 'whole   '}"
                lines.append(f"  {what}  " + ("not measured" if not t else
                             f"{1e3 * statistics.median(t):8.1f} ({1e3 * min(t):.1f} .. {1e3 * max(t):.1f})"))
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
