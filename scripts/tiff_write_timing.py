"""Times the TIFF way out (lbdrn_hip/raster_io.py, lbdrn_hip/tiff_write.py, csrc/tiffw.hip) on the synthetic scenes
scripts/tiff_read_timing.py reads, 8 x 6000 x 6000 and 4 x 7550 x 7550 uint16 (lbdrn_hip.synth.synthetic_tile), with the
planes in HBM at the start of every measurement, written as Deflate, 256 x 256 tiles, planar, predictor 2:

  file size          the writer's segments against zlib level 1 and level 6 on the same segments (the gather stage's bytes)
  (a) baseline       the planes downloaded and written by raster_io.write_raster as before liblbdrn_tiffw.so existed:
                     uncompressed, one strip per band
  (b) the writer     raster_io.write_raster_device, HBM to file
  (c) the host pool  the planes downloaded, each tile differenced and compressed by zlib level 1 on a 16-thread pool, and the
                     same container written
  the device call    lbdrn_tiffw_encode alone, by HIP events, and its gather stage alone (the call with compression 1)

and, first, the rate of ONE 256 KiB segment alone -- one wave, nothing else on the device -- per kind of data.  One warm-up
and --repeats counted runs each; minimum, median and maximum are printed.  Every file written is read back and compared.

    python scripts/tiff_write_timing.py [--sizes 8x6000 4x7550] [--repeats 3] [--rates-only] > profiles/tiff_write_timing.txt
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))

THREADS = 16


def say(*a):
    print(*a, flush=True)


def spread(ts, unit="s"):
    ts = sorted(ts)
    return f"min {ts[0]:.4f} median {ts[len(ts) // 2]:.4f} max {ts[-1]:.4f} {unit} ({len(ts)} runs)"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn, repeats, sync=None):
    out = []
    for run in range(repeats + 1):      # run 0 is the warm-up
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        if run:
            out.append(time.perf_counter() - t0)
    return out


def device_call(planes, lay, repeats):
    """lbdrn_tiffw_encode by HIP events: (seconds of each counted call, body bytes, counts) of the last call"""
    import torch
    from lbdrn_hip import tiff_write
    L = tiff_write.lib()
    dev = planes.device
    nseg = L.lbdrn_tiffw_segment_count(ctypes.byref(lay))
    nws, nout = L.lbdrn_tiffw_workspace(ctypes.byref(lay)), L.lbdrn_tiffw_output_bytes(ctypes.byref(lay))
    out = torch.empty(nout, dtype=torch.uint8, device=dev)
    table = torch.empty(2 * nseg + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    base = table.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ts = []
    for run in range(repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        rc = L.lbdrn_tiffw_encode(ctypes.byref(lay), planes.data_ptr(), out.data_ptr(), nout, base, base + 8 * nseg, base + 16 * nseg,
                                  ws.data_ptr(), nws, stream)
        e[1].record()
        assert rc == 0, L.lbdrn_tiffw_last_error()
        torch.cuda.synchronize(dev)
        if run:
            ts.append(e[0].elapsed_time(e[1]) / 1e3)
    tab = table.cpu().numpy().view(np.uint64)
    return ts, out[:int(tab[2 * nseg])], tab[nseg:2 * nseg].copy()


def layout(tiff_write, shape, compression, tile=256, strip=None):
    C, H, W = shape
    if strip:
        return tiff_write.Layout(C, H, W, 16, 0, 2, W, strip, 0, compression, 2)
    return tiff_write.Layout(C, H, W, 16, 0, 2, tile, tile, 1, compression, 2)


def lone_segment_rates(dev, repeats):
    import torch
    from lbdrn_hip import tiff_write
    from lbdrn_hip.synth import synthetic_tile
    say("== one segment alone (one wave; 1 x 256 x 512 uint16 = 256 KiB in one strip, predictor 2)")
    rng = np.random.default_rng(1)
    kinds = {"scene": synthetic_tile(3, 1, 256, 512), "noise": rng.integers(0, 65536, (1, 256, 512)).astype(np.uint16),
             "constant": np.full((1, 256, 512), 1234, np.uint16)}
    for kind, a in kinds.items():
        planes = torch.from_numpy(a.view(np.int16)).to(dev)
        whole, body, counts = device_call(planes, layout(tiff_write, a.shape, 8, strip=256), repeats)
        gather, raw, _ = device_call(planes, layout(tiff_write, a.shape, 1, strip=256), repeats)
        raw = raw.cpu().numpy().tobytes()
        assert zlib.decompress(body.cpu().numpy().tobytes()) == raw
        t = median(whole) - median(gather)
        say(f"  {kind:8s} stream {int(counts[0]):8d} bytes (zlib -1: {len(zlib.compress(raw, 1)):8d})   call {spread(whole)}   "
            f"gather alone {spread(gather)}   Deflate and pack {t * 1e3:8.2f} ms = {a.nbytes / t / 1e6:7.2f} MB/s of input")


def host_pool_write(path, planes, lay, tiff_write):
    """(c): download, zlib level 1 per tile on the pool, the same container"""
    a = planes.cpu().numpy().view(np.uint16)
    C, H, W = a.shape
    tw, th = lay.seg_w, lay.seg_h
    nx, ny = -(-W // tw), -(-H // th)

    def one(i):
        c, t = divmod(i, nx * ny)
        y0, x0 = (t // nx) * th, (t % nx) * tw
        tile = np.zeros((th, tw), np.uint16)
        part = a[c, y0:y0 + th, x0:x0 + tw]
        tile[:part.shape[0], :part.shape[1]] = part
        d = tile.copy()
        d[:, 1:] -= tile[:, :-1]
        return zlib.compress(d.tobytes(), 1)
    with ThreadPoolExecutor(THREADS) as ex:
        segs = list(ex.map(one, range(C * nx * ny)))
    head, _ = tiff_write.assemble(lay, [len(s) for s in segs])
    with open(path, "wb") as f:
        f.write(head)
        for s in segs:
            f.write(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["8x6000", "4x7550"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rates-only", action="store_true")
    args = ap.parse_args()
    import torch
    from lbdrn_hip import raster_io, tiff_write
    from lbdrn_hip.synth import synthetic_tile
    assert torch.cuda.is_available(), "this script measures on the GPU; it has no CPU fall-back"
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    say(f"device: {torch.cuda.get_device_name(0)}; zlib {zlib.ZLIB_VERSION}; {THREADS} host threads")
    lone_segment_rates(dev, max(args.repeats, 5))
    if args.rates_only:
        return
    tmp = tempfile.mkdtemp(prefix="tiff_write_timing_")
    path = os.path.join(tmp, "scene.tif")
    for size in args.sizes:
        C, side = (int(v) for v in size.split("x"))
        img = synthetic_tile(7, C, side, side)
        planes = torch.from_numpy(img.view(np.int16)).to(dev)
        say(f"== scene {C} x {side} x {side} uint16, synthetic ({img.nbytes} bytes), planes in HBM")
        lay = layout(tiff_write, img.shape, 8)
        whole, body, counts = device_call(planes, lay, args.repeats)
        gather, raw, rcounts = device_call(planes, layout(tiff_write, img.shape, 1), args.repeats)
        raw = raw.cpu().numpy()
        ends = np.cumsum(rcounts).astype(np.int64)
        with ThreadPoolExecutor(THREADS) as ex:
            z1 = sum(ex.map(lambda i: len(zlib.compress(raw[ends[i] - int(rcounts[i]):ends[i]].tobytes(), 1)), range(len(ends))))
            z6 = sum(ex.map(lambda i: len(zlib.compress(raw[ends[i] - int(rcounts[i]):ends[i]].tobytes(), 6)), range(len(ends))))
        del raw
        n = int(body.numel())
        say(f"   {len(counts)} segments; segment bytes: writer {n} ({n / img.nbytes:.4f} of raw), zlib -1 {z1} ({z1 / img.nbytes:.4f}), "
            f"zlib -6 {z6} ({z6 / img.nbytes:.4f}); writer / zlib -1 = {n / z1:.4f}, writer / zlib -6 = {n / z6:.4f}")
        say(f"   lbdrn_tiffw_encode (HIP events)            {spread(whole)} = {img.nbytes / median(whole) / 1e9:.2f} GB/s of input")
        say(f"   its gather stage alone (compression 1)     {spread(gather)}")
        del body
        torch.cuda.empty_cache()
        base = timed(lambda: raster_io.write_raster(path, planes.cpu().numpy().view(np.uint16)), args.repeats, sync)
        say(f"   (a) baseline: download + write_raster      {spread(base)}; file of {os.path.getsize(path)} bytes")
        ours = timed(lambda: raster_io.write_raster_device(path, planes), args.repeats, sync)
        say(f"   (b) write_raster_device (HBM -> file)      {spread(ours)}; file of {os.path.getsize(path)} bytes")
        assert np.array_equal(raster_io.read_raster(path), img), "the written file does not read back to the scene"
        pool = timed(lambda: host_pool_write(path, planes, lay, tiff_write), args.repeats, sync)
        say(f"   (c) download + zlib -1 on {THREADS} threads       {spread(pool)}; file of {os.path.getsize(path)} bytes")
        assert np.array_equal(raster_io.read_raster(path), img), "the host pool's file does not read back to the scene"
        say(f"   (b) / (a) = {median(ours) / median(base):.2f}, (b) / (c) = {median(ours) / median(pool):.2f} (median wall times)")
        del planes
        torch.cuda.empty_cache()
    os.remove(path)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
