"""Times the TIFF front door (lbdrn_hip/raster_io.py, lbdrn_hip/tiff.py, csrc/tiff.hip) on synthetic scenes of the reference's
sizes, 8 x 6000 x 6000 and 4 x 7550 x 7550 uint16 (lbdrn_hip.synth.synthetic_tile), written by tests/tiff_reference.py's
writer in four forms:

  (a) uncompressed, one strip per band             raster_io's own reader, as before liblbdrn_tiff.so existed: the baseline
  (b) Deflate, 256 x 256 tiles, planar, predictor 2
  (c) LZW, one-row strips, chunky, predictor 2     (the writer's LZW encoder is Python: the scene's rows repeat a pool of
                                                    --lzw-pool distinct rows of the scene, each a strip of its own in the file)
  (d) Deflate, one strip per band                  above the segment cap: the host path (the interpreter's zlib)

and, first, the decode rate of ONE segment alone per codec -- one wave, nothing else on the device -- which is what the
segment caps in csrc/tiff.inc are set from: cap = the slowest rate measured here x 0.25 s.

Per form: file bytes; wall time of raster_io.read_raster and read_raster_device (file to array / to HBM); the device call
lbdrn_tiff_decode by HIP events, and k_tiff_place alone by HIP events (a second call that hands the decompressed slots of
the workspace over as an uncompressed file, so that only the placement runs) -- the decompression kernel is the difference;
for the Deflate forms the same bytes inflated by zlib on a 16-thread pool, un-predicted and placed by the pool, ending with
the planes in HBM too.  One warm-up and --repeats counted runs each; minimum, median and maximum are printed.

    python scripts/tiff_read_timing.py [--sizes 8x6000 4x7550] [--repeats 3] [--rates-only] > profiles/tiff_read_timing.txt
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tiff_reference as R  # noqa: E402

THREADS = 16


def say(*a):
    print(*a, flush=True)


def spread(ts, unit="s"):
    ts = sorted(ts)
    return f"min {ts[0]:.4f} median {ts[len(ts) // 2]:.4f} max {ts[-1]:.4f} {unit} ({len(ts)} runs)"


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


def device_call(buf, scene, dev, repeats):
    """(whole lbdrn_tiff_decode call, k_tiff_place alone) in seconds by HIP events, and the planes of the last call"""
    import torch
    from lbdrn_hip import tiff
    L = tiff.lib()
    lay = scene.layout
    nseg = len(scene.offsets)
    nws = L.lbdrn_tiff_workspace(ctypes.byref(lay))
    raw = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    planes = torch.empty((lay.C, lay.H, lay.W), dtype=torch.uint8 if lay.bits == 8 else torch.int16, device=dev)
    status = torch.empty(nseg, dtype=torch.int32, device=dev)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    offsets, counts = np.ascontiguousarray(scene.offsets), np.ascontiguousarray(scene.counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # the second call: the slots of the workspace as an uncompressed file (only k_tiff_place runs)
    plain = tiff.Layout(*[getattr(lay, n) for n, _ in tiff.Layout._fields_])
    plain.compression = tiff.COMP_NONE
    table = (-(-nseg * 8 // 256) * 256) * 2
    seg_bytes = lay.seg_w * lay.seg_h * (1 if lay.planar == 2 else lay.C) * (lay.bits // 8)
    pitch = -(-seg_bytes // 16) * 16
    ws2 = torch.empty(L.lbdrn_tiff_workspace(ctypes.byref(plain)), dtype=torch.uint8, device=dev)
    off2 = np.arange(nseg, dtype=np.uint64) * np.uint64(pitch)
    cnt2 = np.full(nseg, seg_bytes, np.uint64)
    whole, place = [], []
    for run in range(repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        rc = L.lbdrn_tiff_decode(ctypes.byref(lay), raw.data_ptr(), raw.numel(), offsets.ctypes.data, counts.ctypes.data, nseg,
                                 planes.data_ptr(), status.data_ptr(), ws.data_ptr(), nws, stream)
        e[1].record()
        assert rc == 0, L.lbdrn_tiff_last_error()
        torch.cuda.synchronize(dev)
        assert not bool(status.any())
        if lay.compression != tiff.COMP_NONE:
            e[2].record()
            rc = L.lbdrn_tiff_decode(ctypes.byref(plain), ws.data_ptr() + table, nws - table, off2.ctypes.data, cnt2.ctypes.data, nseg,
                                     planes.data_ptr(), status.data_ptr(), ws2.data_ptr(), ws2.numel(), stream)
            e[3].record()
            assert rc == 0, L.lbdrn_tiff_last_error()
            torch.cuda.synchronize(dev)
        if run:
            whole.append(e[0].elapsed_time(e[1]) / 1e3)
            if lay.compression != tiff.COMP_NONE:
                place.append(e[2].elapsed_time(e[3]) / 1e3)
    return whole, place, planes


def lone_segment_rates(dev, repeats):
    """one segment alone on the device, per codec and kind of data: bytes of decompressed output per second of the whole call"""
    import torch
    from lbdrn_hip import tiff
    from lbdrn_hip.synth import synthetic_tile
    say("== one segment alone (one wave; 1 x 256 x 512 uint16 = 256 KiB in one strip, predictor 2 where the codec has one)")
    scene = synthetic_tile(3, 1, 256, 512)
    rng = np.random.default_rng(1)
    kinds = {"scene": scene, "noise": rng.integers(0, 65536, (1, 256, 512)).astype(np.uint16),
             "constant": np.full((1, 256, 512), 1234, np.uint16)}
    slowest = {}
    for comp, name in ((R.COMP_DEFLATE, "Deflate"), (R.COMP_LZW, "LZW"), (R.COMP_PACKBITS, "PackBits")):
        for kind, a in kinds.items():
            for mode in (("dynamic", "fixed", "stored") if comp == R.COMP_DEFLATE and kind == "scene" else ("dynamic",)):
                buf, info = R.write_tiff(a, compression=comp, predictor=2, deflate_mode=mode)
                sc = tiff.parse(buf)
                assert len(sc.offsets) == 1
                whole, place, planes = device_call(buf, sc, dev, repeats)
                assert np.array_equal(planes.cpu().numpy().view(np.uint16), a)
                t = sorted(whole)[len(whole) // 2] - sorted(place)[len(place) // 2]
                rate = a.nbytes / t
                label = f"{name:8s} {kind:8s}" + (f" {mode:7s}" if comp == R.COMP_DEFLATE else "        ")
                say(f"  {label} stream {info['counts'][0]:8d} bytes   call {spread(whole)}   place {spread(place)}   "
                    f"decompression {t * 1e3:8.2f} ms = {rate / 1e6:7.2f} MB/s of output")
                slowest[name] = min(slowest.get(name, rate), rate)
    for name, rate in slowest.items():
        say(f"  {name}: slowest {rate / 1e6:.2f} MB/s -> 0.25 s is {rate * 0.25 / (1 << 20):.2f} MiB; "
            f"lbdrn_tiff_segment_cap = {tiff.lib().lbdrn_tiff_segment_cap({'Deflate': 8, 'LZW': 5, 'PackBits': 32773}[name]) / (1 << 20):.2f} MiB")


def pool_compress(raws, comp):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(lambda r: zlib.compress(r, 6), raws))


def host_pool_read(buf, scene, dev):
    """zlib on a 16-thread pool, each task inflating, un-predicting and placing one segment; then one upload"""
    import torch
    lay = scene.layout
    out = np.empty((lay.C, lay.H, lay.W), np.uint16)
    per_row, rows = -(-lay.W // lay.seg_w), -(-lay.H // lay.seg_h)
    spp = 1 if lay.planar == 2 else lay.C

    def one(i):
        b, t = (i // (per_row * rows), i % (per_row * rows)) if lay.planar == 2 else (None, i)
        y0, x0 = (t // per_row) * lay.seg_h, (t % per_row) * lay.seg_w
        nrows = min(lay.seg_h, lay.H - y0)
        hh = lay.seg_h if lay.tiled else nrows
        o, c = int(scene.offsets[i]), int(scene.counts[i])
        seg = np.frombuffer(zlib.decompress(buf[o:o + c]), "<u2", hh * lay.seg_w * spp).reshape(hh, lay.seg_w, spp)
        if lay.predictor == 2:
            seg = np.cumsum(seg, axis=1, dtype=np.uint16)
        cols = min(lay.seg_w, lay.W - x0)
        dst = out[b:b + 1] if b is not None else out
        dst[:, y0:y0 + nrows, x0:x0 + cols] = seg[:nrows, :cols, :].transpose(2, 0, 1)
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(one, range(len(scene.offsets))))
    return torch.from_numpy(out.view(np.int16)).to(dev)


def scene_forms(img, lzw_pool):
    """[(label, file bytes)] -- built one at a time by the caller to bound the memory in use"""
    C, H, W = img.shape

    def form_a():
        return R.write_tiff(img, planar=2)[0]

    def form_b():
        raw = R.raw_segments(img, tile=(256, 256), planar=2, predictor=2)
        return R.write_tiff(img, tile=(256, 256), planar=2, predictor=2, compression=R.COMP_DEFLATE, raw=raw, packed=pool_compress(raw, 8))[0]

    def form_c():
        pool = [R.lzw_encode(r) for r in R.raw_segments(img[:, :lzw_pool], rows_per_strip=1, planar=1, predictor=2)]
        packed = [pool[y % lzw_pool] for y in range(H)]
        return R.write_tiff(img, rows_per_strip=1, planar=1, predictor=2, compression=R.COMP_LZW, raw=[b""] * H, packed=packed)[0]

    def form_d():
        raw = R.raw_segments(img, planar=2, predictor=2)
        return R.write_tiff(img, planar=2, predictor=2, compression=R.COMP_DEFLATE, raw=raw, packed=pool_compress(raw, 8))[0]
    return (("(a) uncompressed, one strip per band", form_a, None), ("(b) Deflate, 256 x 256 tiles, planar, predictor 2", form_b, None),
            (f"(c) LZW, one-row strips, chunky, predictor 2 (rows repeat the scene's first {lzw_pool})", form_c, lzw_pool),
            ("(d) Deflate, one strip per band, predictor 2 (host path)", form_d, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["8x6000", "4x7550"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lzw-pool", type=int, default=48)
    ap.add_argument("--rates-only", action="store_true")
    args = ap.parse_args()
    import torch
    from lbdrn_hip import raster_io, tiff
    from lbdrn_hip.synth import synthetic_tile
    assert torch.cuda.is_available(), "this script measures on the GPU; it has no CPU fall-back"
    dev = torch.device("cuda:0")
    say(f"device: {torch.cuda.get_device_name(0)}; zlib {zlib.ZLIB_VERSION}; {THREADS} host threads")
    lone_segment_rates(dev, max(args.repeats, 5))
    if args.rates_only:
        return
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    tmp = tempfile.mkdtemp(prefix="tiff_timing_")
    for size in args.sizes:
        C, side = (int(v) for v in size.split("x"))
        t0 = time.perf_counter()
        img = synthetic_tile(7, C, side, side)
        say(f"== scene {C} x {side} x {side} uint16, synthetic ({img.nbytes} bytes; generated in {time.perf_counter() - t0:.1f} s)")
        for label, make, pool in scene_forms(img, args.lzw_pool):
            t0 = time.perf_counter()
            buf = make()
            path = os.path.join(tmp, "scene.tif")
            with open(path, "wb") as f:
                f.write(buf)
            say(f"-- {label}: file of {len(buf)} bytes ({img.nbytes / len(buf):.2f} : 1; written in {time.perf_counter() - t0:.1f} s)")
            want = img if pool is None else np.concatenate([img[:, :pool]] * -(-side // pool), axis=1)[:, :side]
            got = raster_io.read_raster(path)
            assert np.array_equal(got, want), "read_raster differs from the scene"
            del got
            say(f"   read_raster (file -> numpy)        {spread(timed(lambda: raster_io.read_raster(path), args.repeats))}")
            say(f"   read_raster_device (file -> HBM)   {spread(timed(lambda: raster_io.read_raster_device(path, dev), args.repeats, sync))}")
            sc = tiff.parse(buf, path)
            route = "device"
            if sc.layout.compression != tiff.COMP_NONE and tiff._over_cap(sc.layout, path) == "host":
                route = "host (a segment is above the cap)"
            say(f"   route: {route}; {len(sc.offsets)} segments")
            if route == "device" and not (sc.plain_strips() and buf[2:4] == b"*\0"):
                whole, place, planes = device_call(buf, sc, dev, args.repeats)
                assert np.array_equal(planes.cpu().numpy().view(np.uint16), want)
                del planes
                say(f"   lbdrn_tiff_decode (HIP events)     {spread(whole)}")
                if place:
                    w, p = sorted(whole)[len(whole) // 2], sorted(place)[len(place) // 2]
                    say(f"   k_tiff_place alone (HIP events)    {spread(place)}")
                    say(f"   decompression kernel (difference)  {w - p:.4f} s = {img.nbytes / (w - p) / 1e9:.2f} GB/s of output, "
                        f"{(w - p) / len(sc.offsets) * 1e6:.2f} us a segment amortised")
            if sc.layout.compression == tiff.COMP_DEFLATE:
                t = host_pool_read(buf, sc, dev)
                assert np.array_equal(t.cpu().numpy().view(np.uint16), want)
                del t
                say(f"   zlib on {THREADS} host threads -> HBM     {spread(timed(lambda: host_pool_read(buf, sc, dev), args.repeats, sync))}")
            del buf
            torch.cuda.empty_cache()
    os.remove(os.path.join(tmp, "scene.tif"))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
