"""Times the overview pyramid (lbdrn_hip/pyramid.py, csrc/pyramid.hip) and the pyramidal write (lbdrn_hip/tiff_write.py) on the
synthetic scene scripts/tiff_write_timing.py writes, 8 x 6000 x 6000 uint16 (lbdrn_hip.synth.synthetic_tile), with the planes
in HBM at the start of every measurement; Deflate, 256 x 256 tiles, planar, predictor 2, overviews "auto" (5 levels):

  --part events   lbdrn_pyr_build alone, by HIP events: all levels in one call, average, average with nodata and nearest; and
                  level by level (a call of one level from the level before it), with the bytes each moves
  --part wall     raster_io.write_raster_device without overviews -- the write as it was before the options existed: the same
                  code path, liblbdrn_tiffw.so is untouched -- against the same call with overviews="auto"; file sizes; and the
                  pyramidal write taken apart: the reduction, each level's encode_device, the container and the file

One warm-up and --repeats counted runs each; minimum, median and maximum are printed.  The pyramidal file is read back level
by level and compared with a numpy reduction of the scene.  Run each part under a time limit of its own:

    timeout -k 10 300 python scripts/pyramid_timing.py --part events >  profiles/pyramid_timing.txt
    timeout -k 10 600 python scripts/pyramid_timing.py --part wall   >> profiles/pyramid_timing.txt
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))


def say(*a):
    print(*a, flush=True)


def spread(ts, unit="s"):
    ts = sorted(ts)
    return f"min {ts[0]:.5f} median {ts[len(ts) // 2]:.5f} max {ts[-1]:.5f} {unit} ({len(ts)} runs)"


def median(ts):
    return sorted(ts)[len(ts) // 2]


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


def reduce_numpy(a):
    """one average level of [C,H,W] uint16 in numpy (even sides only: the scene's levels down to 375 are checked with it)"""
    v = a.astype(np.uint32)
    s = v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
    return ((s + 2) >> 2).astype(np.uint16)


def events(planes, levels, repeats, resampling=0, nodata=None, src_shape=None):
    """lbdrn_pyr_build by HIP events: seconds of each counted call"""
    import torch
    from lbdrn_hip import pyramid
    L = pyramid.lib()
    C, H, W = planes.shape
    d = pyramid.Desc(C, H, W, 16, resampling, nodata is not None, nodata or 0, 0, planes.stride(1), planes.stride(0))
    nout = L.lbdrn_pyr_output_bytes(ctypes.byref(d), levels)
    out = torch.empty(nout, dtype=torch.uint8, device=planes.device)
    stream = torch.cuda.current_stream(planes.device).cuda_stream
    ts = []
    for run in range(repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        rc = L.lbdrn_pyr_build(ctypes.byref(d), planes.data_ptr(), levels, out.data_ptr(), nout, stream)
        e[1].record()
        assert rc == 0, L.lbdrn_pyr_last_error()
        torch.cuda.synchronize(planes.device)
        if run:
            ts.append(e[0].elapsed_time(e[1]) / 1e3)
    return ts, nout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["events", "wall"], required=True)
    ap.add_argument("--size", default="8x6000")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from lbdrn_hip import pyramid, raster_io, tiff_write
    from lbdrn_hip.synth import synthetic_tile
    assert torch.cuda.is_available(), "this script measures on the GPU; it has no CPU fall-back"
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    C, side = (int(v) for v in args.size.split("x"))
    img = synthetic_tile(7, C, side, side)
    planes = torch.from_numpy(img.view(np.int16)).to(dev)
    sizes = pyramid.level_sizes(side, side, "auto")
    say(f"== {args.part}: device {torch.cuda.get_device_name(0)}; scene {C} x {side} x {side} uint16, synthetic ({img.nbytes} bytes), planes in HBM; "
        f"overviews auto: {len(sizes)} levels {[w for _, w in sizes]}")
    if args.part == "events":
        for name, resampling, nodata in (("average", 0, None), ("average, nodata 0", 0, 0), ("nearest", 1, None)):
            ts, nout = events(planes, len(sizes), args.repeats, resampling, nodata)
            moved = img.nbytes * (1 if resampling == 0 else 0.25) + nout * 1.25      # level 0 read, every level written, all but the last read
            say(f"   lbdrn_pyr_build, {len(sizes)} levels, {name:18s} {spread(ts)} = {moved / median(ts) / 1e9:7.1f} GB/s of bytes moved "
                f"({nout} output bytes)")
        src = planes
        for k, (h, w) in enumerate(sizes, 1):
            ts, nout = events(src, 1, args.repeats)
            say(f"   level {k} alone ({h} x {w} from {src.shape[1]} x {src.shape[2]}), average   {spread(ts)} = "
                f"{(src.numel() * 2 + nout) / median(ts) / 1e9:7.1f} GB/s of bytes moved")
            src = pyramid.build(src, 1)[0]
        return
    tmp = tempfile.mkdtemp(prefix="pyramid_timing_")
    path = os.path.join(tmp, "scene.tif")
    plain = timed(lambda: raster_io.write_raster_device(path, planes), args.repeats, sync)
    plain_size = os.path.getsize(path)
    say(f"   write_raster_device, no overviews (the write as it was)   {spread(plain)}; file of {plain_size} bytes")
    pyr = timed(lambda: raster_io.write_raster_device(path, planes, overviews="auto"), args.repeats, sync)
    pyr_size = os.path.getsize(path)
    say(f"   write_raster_device, overviews='auto'                      {spread(pyr)}; file of {pyr_size} bytes")
    say(f"   ratio of the median wall times {median(pyr) / median(plain):.3f}; ratio of the file sizes {pyr_size / plain_size:.3f}; "
        f"ratio of the samples {1 + sum(h * w for h, w in sizes) / (side * side):.3f}")
    want = img
    for k in range(1, len(sizes) + 1):
        got = raster_io.read_raster(path, overview=k)
        if want.shape[1] % 2 == 0 and want.shape[2] % 2 == 0:
            want = reduce_numpy(want)
            assert np.array_equal(got, want), f"level {k} does not read back to the numpy reduction"
        else:
            want = got
    assert np.array_equal(raster_io.read_raster(path), img), "level 0 does not read back to the scene"
    # the pyramidal write taken apart
    lays = [tiff_write.make_layout(C, h, w, 16, "deflate") for h, w in [(side, side)] + sizes]
    build = timed(lambda: pyramid.build(planes, len(sizes)), args.repeats, sync)
    say(f"   parts: pyramid.build (allocation, launches, sync)          {spread(build)}")
    levels = [planes] + pyramid.build(planes, len(sizes))
    kept = []
    for k, (t, lay) in enumerate(zip(levels, lays)):
        ts = timed(lambda: kept.__setitem__(slice(k, k + 1), [tiff_write.encode_device(t, lay)]), args.repeats, sync)
        say(f"   parts: encode_device of level {k} ({lay.H} x {lay.W}, {tiff_write.segment_count(lay)} segments)   {spread(ts)}")

    def container():
        head, _ = tiff_write.assemble_pyramid(lays, [c for _, _, c in kept])
        with open(path, "wb") as f:
            f.write(head)
            for body, _, _ in reversed(kept):
                f.write(memoryview(body))
    ts = timed(container, args.repeats, sync)
    say(f"   parts: assemble_pyramid and the file                        {spread(ts)}")
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
