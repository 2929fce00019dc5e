"""What `encode.py --nodata V` costs and saves on one full-size tile, beside the same commands without the flag on this commit
and on the parent commit.

The tile is the 8 x 2048^2 synthetic one with a collar set to 0: everything outside the largest square that fits the frame
when turned by 12 degrees (29 % of the plane), the shape an orthorectified scene has.  Four encodes -- with and without
`--nodata 0`, each with and without `--max-error 0` -- and the whole decode of each file.  Every measurement is the wall time
of encode.main() / decode.main(), file read to file written, in a process that has run the same command once before;
processes of the two trees alternate.  Beside the times: the file sizes and the bytes of the mask chunk.

    python scripts/nodata_timing.py [--parent DIR] [--out profiles/nodata_timing.txt] [--small]

--parent: the lbdrn-msic_amd directory of a checkout of the parent commit with its libraries built (`git worktree add`, then
build); without it the parent rows read "not measured"."""
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
REPS = 3
JOBS = {"plain": [], "nodata": ["--nodata", "0"], "plain T=0": ["--max-error", "0"], "nodata T=0": ["--nodata", "0", "--max-error", "0"]}


def collared_tile(side):
    """the synthetic tile with 0 outside the inscribed square turned by 12 degrees -> (raster, the collar's share)"""
    import numpy as np
    sys.path.insert(0, BRANCH)
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(0, 8, side, side).astype(np.uint16)
    img[img == 0] = 1
    t = np.deg2rad(12.0)
    half = side / (np.cos(t) + np.sin(t)) / 2
    yy, xx = np.mgrid[0:side, 0:side] - (side - 1) / 2
    u, v = xx * np.cos(t) + yy * np.sin(t), -xx * np.sin(t) + yy * np.cos(t)
    collar = (np.abs(u) > half) | (np.abs(v) > half)
    img[:, collar] = 0
    return img, float(collar.mean())


def worker(tree, src, workdir, labels):
    """-> one JSON line {label: {"encode": [s, ...], "decode": [s, ...], "bytes": n, "mask": n or None}}"""
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
            size, mask = os.path.getsize(binp), None
            if "--nodata" in JOBS[label]:
                from lbdrn_hip import container
                with open(binp, "rb") as f:
                    mask = len(container.pack_nodata_trailer(*container.unpack_nodata_trailer(f.read())))
            shutil.rmtree(root)                           # (a .bin and a 64 MB raster per run)
        out[label] = {"encode": enc[1:], "decode": dec[1:], "bytes": size, "mask": mask}
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "nodata_timing.txt"))
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
            trees = ([("parent", args.parent, ["plain", "plain T=0"])] if args.parent else []) + [("branch", BRANCH, list(JOBS))]
            for who, tree, labels in trees:
                for label, rec in run_worker(tree, src, d, labels).items():
                    have = got.setdefault((who, label), {"encode": [], "decode": [], "bytes": rec["bytes"], "mask": rec["mask"]})
                    have["encode"] += rec["encode"]
                    have["decode"] += rec["decode"]
                    assert have["bytes"] == rec["bytes"] and have["mask"] == rec["mask"]
    ms = lambda t: f"{1e3 * statistics.median(t):8.1f} ({1e3 * min(t):.1f} .. {1e3 * max(t):.1f})"
    lines = [f"8 x {side} x {side} synthetic tile, collar of {100 * share:.1f} % set to 0, -sr 1, K5 D2 bc64 nl2 e10, LBB2; wall time of "
             f"encode.main / decode.main, ms, median (min .. max) of {2 * REPS} runs in 2 processes; sizes in bytes",
             f"  {'':6s} {'':12s} {'encode.main':>30s} {'decode.main':>30s} {'file':>12s} {'mask chunk':>12s} {'bpsp':>8s}"]
    for who in ("parent", "branch"):
        for label in JOBS:
            rec = got.get((who, label))
            if rec is None:
                if who == "parent" and "nodata" not in label:
                    lines.append(f"  {who:6s} {label:12s} not measured")
                continue
            lines.append(f"  {who:6s} {label:12s} {ms(rec['encode']):>30s} {ms(rec['decode']):>30s} {rec['bytes']:12d} "
                         f"{rec['mask'] if rec['mask'] is not None else '-':>12} {rec['bytes'] * 8 / (8 * side * side):8.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if not args.small:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
