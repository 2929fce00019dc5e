"""Times the GPU JPEG 2000 decoder (lbdrn_hip/jp2k_dec.py, csrc/jp2k_dec.hip) against OpenJPEG on 8 threads, the two
readers alternating in one process, three counted runs each after a warm-up (as profiles/jp2_gpu_timing.txt was made):

  * the bare decode call of the headline tile's MSB planes (8 x 2048 x 2048, K = 5) and of the 8 x 6000 x 6000 scene,
    both written by jp2-gpu; the GPU figure is lbdrn_jp2kd_decode with the planes left in HBM, OpenJPEG's is
    lbdrn_jp2_decode into host memory (the copy to the device the apply pass then needs is timed separately);
  * decode.main file to file on a jp2-gpu .bin, LBDRN_BASE_DECODER=gpu against LBDRN_BASE_DECODER=openjpeg (the reader
    the parent commit always takes: the same code path as before this decoder existed).

    python scripts/jp2k_decode_timing.py [--scene 6000] [--skip-cli] > profiles/jp2k_gpu_decode_timing.txt

The per-kernel split comes from one run under the profiler:
    rocprofv3 --kernel-trace --stats -d runs/jp2k_dec -o jp2k_dec -- python scripts/jp2k_decode_timing.py --profile-only
    (the *_kernel_stats.csv it writes is profiles/jp2k_gpu_decode_kernel_stats.csv)
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))


def bare(label, x, dev, have_openjpeg):
    import torch
    from lbdrn_hip import container, jp2, jp2k_dec, ops
    f = container.encode_base(x, codec="jp2-gpu", device=dev)
    print(f"{label}: {x.shape} uint16, file of {len(f)} bytes", flush=True)
    times = {"gpu": [], "openjpeg": [], "openjpeg+h2d": []}
    for run in range(4):      # run 0 is the warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        planes, bits = jp2k_dec.decode(f, dev)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if run == 0:
            assert np.array_equal(planes.cpu().numpy().view(np.uint16), x), "the GPU decoder does not return the planes"
        del planes
        if run:
            times["gpu"].append(t1 - t0)
        if have_openjpeg:
            t0 = time.perf_counter()
            y = jp2.decode(f)
            t1 = time.perf_counter()
            t = ops.to_device_u16(y, dev)
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            if run == 0:
                assert np.array_equal(y, x)
            del t, y
            if run:
                times["openjpeg"].append(t1 - t0)
                times["openjpeg+h2d"].append(t2 - t0)
    for k, v in times.items():
        if v:
            print(f"  {k:13s} {' '.join(f'{1e3 * s:9.1f}' for s in v)} ms   (median {1e3 * sorted(v)[1]:.1f} ms)", flush=True)


def cli(dev):
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(0, 8, 2048, 2048)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "tile.tif")
        raster_io.write_raster(src, img)
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lbdrn-msic_amd"), LBDRN_BASE_CODEC="jp2-gpu")
        subprocess.run([sys.executable, os.path.join(ROOT, "lbdrn-msic_amd", "encode.py"), "-i", src, "-o", tmp, "-K", "5", "-D", "2", "-bs", "512", "-e", "1", "-sr", "1"],
                       check=True, env=env, capture_output=True)
        bins = [os.path.join(d, n) for d, _, names in os.walk(tmp) for n in names if n.endswith(".bin")]
        assert len(bins) == 1, bins
        print(f"decode.py file to file, 8 x 2048 x 2048, K = 5, jp2-gpu payload ({os.path.getsize(bins[0])} bytes), a process per run", flush=True)
        times = {"gpu": [], "openjpeg": []}
        for run in range(4):
            for reader in ("gpu", "openjpeg"):
                e = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lbdrn-msic_amd"), LBDRN_BASE_DECODER=reader, LBDRN_JP2_THREADS="8")
                t0 = time.perf_counter()
                subprocess.run([sys.executable, os.path.join(ROOT, "lbdrn-msic_amd", "decode.py"), "-i", bins[0]], check=True, env=e, capture_output=True)
                if run:
                    times[reader].append(time.perf_counter() - t0)
        for k, v in times.items():
            print(f"  LBDRN_BASE_DECODER={k:9s} {' '.join(f'{s:7.2f}' for s in v)} s   (median {sorted(v)[1]:.2f} s)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=6000)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    import torch
    from lbdrn_hip import jp2
    from lbdrn_hip.synth import synthetic_tile
    dev = torch.device("cuda:0")
    if a.profile_only:
        from lbdrn_hip import container, jp2k_dec
        f = container.encode_base(np.ascontiguousarray(synthetic_tile(0, 8, 2048, 2048) >> 5), codec="jp2-gpu", device=dev)
        for _ in range(3):
            jp2k_dec.decode(f, dev)
        return 0
    have = jp2.available()
    if have:
        jp2.set_threads(8)
    print(f"device {torch.cuda.get_device_name(dev)}; OpenJPEG {'on 8 threads' if have else 'absent'}", flush=True)
    bare("headline tile", np.ascontiguousarray(synthetic_tile(0, 8, 2048, 2048) >> 5), dev, have)
    if a.scene:
        bare("scene", np.ascontiguousarray(synthetic_tile(0, 8, a.scene, a.scene) >> 5), dev, have)
    if not a.skip_cli:
        cli(dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
