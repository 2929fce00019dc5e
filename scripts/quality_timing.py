"""Timing of the quality report (lbdrn_hip.quality, liblbdrn_quality.so) against the three numpy expressions of decode.py's
`-org` records, on 8 x 2048 x 2048 and 8 x 6000 x 6000 uint16 rasters (b = a with its low 5 bits redrawn).

    python scripts/quality_timing.py [--out profiles/quality_timing.txt] [--runs 3] [--small-only]

Per raster, one warm-up and --runs counted runs of each line, the median and the spread (min .. max) printed:
    numpy on host arrays           np.mean((a.astype(f32) - b.astype(f32)) ** 2), the PSNR from it, and
                                   np.abs(a.astype(i64) - b.astype(i64)).max(): what decode.py computes without --metrics
    compare, host arrays           quality.compare(a, b) from numpy arrays: upload, kernels, download of the result
    compare, planes in HBM         quality.compare on tensors that already lie in HBM, host clock, ending in the download
    device time, what = 0 / SAM / SSIM / both   lbdrn_quality_compare alone between two HIP events
The statistics + SAM pass is what = SAM (the memset and the last launch included); it must read both rasters once, and its
rate is 2 x raster bytes over its time.  The SSIM pass is what = SSIM minus what = 0 (both run the statistics pass).
Needs a GPU; nothing here falls back to the CPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))


def spread(ts):
    return f"{statistics.median(ts) * 1e3:10.3f} ms  ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def numpy_way(a, b):
    mse = np.mean((a.astype(np.float32) - b.astype(np.float32)) ** 2)
    psnr = 10 * np.log10(10000 ** 2 / mse)
    mx = int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max())
    return mse, psnr, mx


def main():
    import torch
    from lbdrn_hip import ops, quality
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_timing.txt"))
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--small-only", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "quality_timing.py measures on the GPU"
    dev = torch.device("cuda:0")
    L = quality.lib()
    lines = [f"quality_timing.py: {torch.cuda.get_device_name(0)}, one warm-up and {args.runs} counted runs a line: median (min .. max)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    for shape in ((8, 2048, 2048),) + (() if args.small_only else ((8, 6000, 6000),)):
        C, H, W = shape
        rng = np.random.default_rng(1)
        a = rng.integers(0, 65536, shape, dtype=np.uint16)
        b = (a & np.uint16(0xFFE0)) | rng.integers(0, 32, shape, dtype=np.uint16)
        nbytes = 2 * a.nbytes
        emit(f"\n{C} x {H} x {W} uint16, {a.nbytes / 1e6:.0f} MB a raster")

        def timed(fn):
            fn()
            ts = []
            for _ in range(args.runs):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t0)
            return ts
        emit(f"  numpy on host arrays (MSE, PSNR, max error)   {spread(timed(lambda: numpy_way(a, b)))}")
        emit(f"  compare, host arrays (upload included)        {spread(timed(lambda: quality.compare(a, b)))}")
        ta, tb = ops.to_device_u16(a, dev), ops.to_device_u16(b, dev)
        emit(f"  compare, planes in HBM                        {spread(timed(lambda: quality.compare(ta, tb)))}")
        q = quality.compare(ta, tb)
        mse, _, mx = numpy_way(a, b)
        assert q.overall.max_abs == mx and abs(q.overall.mse - float(mse)) <= 1e-5 * q.overall.mse, (q.overall.mse, mse, mx)
        result = torch.empty(L.lbdrn_quality_result_bytes(C) // 8, dtype=torch.int64, device=dev)
        dt = {}
        for what, name in ((0, "statistics alone"), (quality.SAM, "statistics + SAM"), (quality.SSIM, "statistics, SSIM"), (3, "all")):
            nws = L.lbdrn_quality_workspace(C, H, W, what)
            ws = torch.empty(max(nws, 8) // 8, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream

            def call():
                rc = L.lbdrn_quality_compare(ta.data_ptr(), W, H * W, tb.data_ptr(), W, H * W, 16, C, H, W, 10000.0, what, result.data_ptr(),
                                             ws.data_ptr(), nws, stream)
                assert rc == 0, L.lbdrn_quality_last_error()
            call()
            torch.cuda.synchronize(dev)
            ts = []
            for _ in range(max(args.runs, 5)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            dt[what] = ts
            rate = f"   {nbytes / statistics.median(ts) / 1e12:.2f} TB/s of the 2 x raster it reads" if what in (0, quality.SAM) else ""
            emit(f"  device time, what = {what} ({name:<17})       {spread(ts)}{rate}")
        emit(f"  SSIM pass (what = SSIM minus what = 0), medians {1e3 * (statistics.median(dt[quality.SSIM]) - statistics.median(dt[0])):10.3f} ms")
        del ta, tb
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
