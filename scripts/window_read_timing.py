"""Times reading a window of a scene (raster_io.read_raster_device(path, window=), lbdrn_hip.tiff.read_window_bytes) beside the
whole read, on this commit and on the parent commit (`--parent DIR`: the lbdrn-msic_amd directory of a built checkout of
it, where a window is the whole read, sliced).  The synthetic 8 x 6000 x 6000 uint16 scene of scripts/tiff_read_timing.py
in three forms: (b) Deflate 256 x 256 tiles, (c) LZW one-row strips, (a) uncompressed, one strip per band.

Per form and commit, each in a process of its own, this commit first, one warm-up and --repeats counted runs an item:

  the whole read                read_raster_device, file -> HBM
  a 512 x 512 window            at the centre and at the corner: wall time file -> HBM, the bytes uploaded and the segments
                                decoded (tiff.plan_window: the touched segments and no others; the uncompressed strips are
                                read on the host, rows from the memory map, and only the window is uploaded)
  encode.py -sr 4 -e 2          encode.main, file -> .bin; on this commit also under LBDRN_TILE_READS=1 (same .bin: checked)
  decode.py --window ... -org   decode.main of that .bin, the centre window, compared with the original

Every window is compared with the slice of the whole read before it is timed.  Wall times end in a device synchronise.

    python scripts/window_read_timing.py [--parent DIR] [--repeats 3] [--forms b c a] > profiles/window_read_timing.txt
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, BANDS, WIN = 6000, 8, 512
WINDOWS = (("centre", ((SIDE - WIN) // 2, (SIDE - WIN) // 2, WIN, WIN)), ("corner", (0, 0, WIN, WIN)))
ENCODE = ["-sr", "4", "-e", "2", "-K", "5"]


def say(*a):
    print(*a, flush=True)


def spread(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.4f} median {ts[len(ts) // 2]:.4f} max {ts[-1]:.4f} s ({len(ts)} runs)"


def timed(fn, repeats, sync):
    out = []
    for run in range(repeats + 1):      # run 0 is the warm-up
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if run:
            out.append(time.perf_counter() - t0)
    return out


# ---------------------------------------------------------------- one commit, one file: a process of its own

def child(tree, path, repeats, work):
    sys.path.insert(0, tree)
    import contextlib
    import io
    import torch
    import decode
    import encode
    from lbdrn_hip import raster_io, tiff
    assert torch.cuda.is_available(), "this script measures on the GPU; it has no CPU fall-back"
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    windows = hasattr(tiff, "plan_window")
    out = {"windows": windows}
    full = raster_io.read_raster_device(path, dev)
    out["whole read"] = timed(lambda: raster_io.read_raster_device(path, dev), repeats, sync)
    with open(path, "rb") as f:
        buf = f.read()
    try:
        scene = tiff.parse(buf, path)
    except ValueError:
        scene = None
    plain = scene is not None and scene.plain_strips() and buf[2:4] in (b"*\0", b"\0*")
    for name, (x0, y0, w, h) in WINDOWS:
        if windows:
            read = lambda: raster_io.read_raster_device(path, dev, window=(x0, y0, w, h))      # noqa: E731
            if plain:
                note = f"{BANDS * h * SIDE * 2} bytes of rows read on the host, {BANDS * h * w * 2} uploaded, no segment decoded"
            else:
                plan = tiff.plan_window(scene, (x0, y0, w, h))
                assert plan.nbytes == sum(int(scene.counts[i]) for i in set(plan.segments))
                note = f"{plan.nbytes} bytes uploaded, {len(plan.segments)} of {len(scene.offsets)} segments decoded"
        else:
            read = lambda: raster_io.read_raster_device(path, dev)[:, y0:y0 + h, x0:x0 + w].contiguous()      # noqa: E731
            note = f"{len(buf)} bytes " + ("read on the host" if plain else f"uploaded, {len(scene.offsets)} segments decoded")
        assert torch.equal(read(), full[:, y0:y0 + h, x0:x0 + w]), "the window differs from the slice"
        out[f"window {name}"] = (timed(read, repeats, sync), note)
    del full, buf
    torch.cuda.empty_cache()

    def quiet(fn, argv):
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            assert fn(argv, shard_tiles=False) == 0

    def encode_runs(label, env):
        os.environ.pop("LBDRN_TILE_READS", None)
        os.environ.update(env)
        ts, bins = [], None
        for run in range(repeats + 1):
            out_dir = os.path.join(work, f"enc_{label}")
            shutil.rmtree(out_dir, ignore_errors=True)
            sync()
            t0 = time.perf_counter()
            quiet(encode.main, ["-i", path, "-o", out_dir] + ENCODE)
            sync()
            if run:
                ts.append(time.perf_counter() - t0)
            (sub,) = os.listdir(out_dir)
            bins = os.path.join(out_dir, sub, "scene.bin")
        os.environ.pop("LBDRN_TILE_READS", None)
        return ts, bins
    out["encode -sr 4"], bin_path = encode_runs("default", {})
    if windows:
        out["encode -sr 4, LBDRN_TILE_READS=1"], other = encode_runs("tiles", {"LBDRN_TILE_READS": "1"})
        with open(bin_path, "rb") as a, open(other, "rb") as b:
            assert a.read() == b.read(), "LBDRN_TILE_READS=1 wrote another .bin"
    x0, y0, w, h = WINDOWS[0][1]
    argv = ["-i", bin_path, "--window", str(x0), str(y0), str(w), str(h), "-o", os.path.join(work, "w.tif"), "-org", path]
    out["decode --window -org"] = timed(lambda: quiet(decode.main, argv), repeats, sync)
    print("@@" + json.dumps(out), flush=True)


# ---------------------------------------------------------------- the driver

def forms(img, lzw_pool):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import tiff_read_timing as T
    a, b, c, _ = T.scene_forms(img, lzw_pool)
    return {"a": a, "b": b, "c": c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, metavar="DIR", help="lbdrn-msic_amd of a built checkout of the parent commit")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", nargs="*", default=["b", "c", "a"])
    ap.add_argument("--lzw-pool", type=int, default=48)
    ap.add_argument("--child", nargs=3, default=None, metavar=("TREE", "FILE", "WORK"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.repeats, args.child[2])
    sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from lbdrn_hip.synth import synthetic_tile
    assert torch.cuda.is_available(), "this script measures on the GPU; it has no CPU fall-back"
    say(f"device: {torch.cuda.get_device_name(0)}; scene {BANDS} x {SIDE} x {SIDE} uint16, synthetic; windows of {WIN} x {WIN}; "
        f"encode.py {' '.join(ENCODE)}; one warm-up and {args.repeats} counted runs an item, a process per commit and form")
    if args.parent is None:
        say("no --parent: this commit only")
    img = synthetic_tile(7, BANDS, SIDE, SIDE)
    work = tempfile.mkdtemp(prefix="window_timing_")
    path = os.path.join(work, "scene.tif")
    trees = [("this commit", os.path.join(ROOT, "lbdrn-msic_amd"))] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    for key in args.forms:
        label, make, _ = forms(img, args.lzw_pool)[key]
        with open(path, "wb") as f:
            f.write(make())
        say(f"== {label}: file of {os.path.getsize(path)} bytes")
        results = {}
        for name, tree in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--child", tree, path, work],
                               capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests")))
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("@@")]
            if p.returncode or not lines:
                say(f"   {name}: FAILED (exit status {p.returncode})\n{p.stderr[-2000:]}")
                return 1
            results[name] = json.loads(lines[-1][2:])
        for item in results["this commit"]:
            if item == "windows":
                continue
            for name, _ in trees:
                r = results[name].get(item)
                if r is None:
                    continue
                ts, note = (r[0], "; " + r[1]) if isinstance(r[0], list) else (r, "")
                whole = " (the whole read, sliced)" if item.startswith("window") and not results[name]["windows"] else ""
                say(f"   {item:34s} {name:12s} {spread(ts)}{note}{whole}")
    shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
