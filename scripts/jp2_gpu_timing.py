"""The reference-format MSB payload coded on the GPU (LBDRN_BASE_CODEC=jp2-gpu, csrc/jp2k.hip) against the host codec it
stands beside: encode.main's wall time file to file with the default LBB2 payload, with jp2 (OpenJPEG on 8 host threads,
coded beside the fits) and with jp2-gpu, alternating, several times each, in one process -- on one 8 x 2048^2 tile and, with
`scene`, on the 8 x 6000 x 6000 scene at -sr 1; then the bare lbdrn_jp2k_encode call between device synchronisations.
    python scripts/jp2_gpu_timing.py [scene] [--repeats N] [--out profiles/jp2_gpu_timing.txt]"""
import os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))
import numpy as np
import torch
import encode
from lbdrn_hip import jp2, ops, raster_io
from lbdrn_hip.synth import synthetic_tile

argv = sys.argv[1:]
repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


cases = [("tile", 2048, 0)] + ([("scene", 6000, 7)] if "scene" in argv else [])
say(f"host threads available {len(os.sched_getaffinity(0))}, OpenJPEG worker threads {jp2.default_threads()}, "
    f"{torch.cuda.get_device_name(0)}, {repeats} runs of each codec, alternating")
os.environ["LBDRN_JP2_AHEAD"] = "1"
with tempfile.TemporaryDirectory() as d:
    warm = os.path.join(d, "warm.npy")
    raster_io.write_raster(warm, synthetic_tile(1, 8, 128, 128))
    for codec_name in ("LBB2", "jp2", "jp2-gpu"):
        encode.BASE_CODEC = codec_name
        encode.main(["-i", warm, "-o", os.path.join(d, "w_" + codec_name)])
    for name, side, seed in cases:
        img = synthetic_tile(seed, 8, side, side)
        src = os.path.join(d, f"{name}.npy")
        raster_io.write_raster(src, img)
        times, size = {}, {}
        for rep in range(repeats + 1):          # (run 0 of each codec warms this geometry up and is not counted)
            for codec_name in ("LBB2", "jp2", "jp2-gpu"):
                encode.BASE_CODEC = codec_name
                out = os.path.join(d, f"o_{name}_{codec_name}_{rep}")
                torch.cuda.synchronize()
                t0 = time.time()
                encode.main(["-i", src, "-o", out])
                te = time.time() - t0
                log = open(os.path.join(out, f"{name}_r1_K5_bc64_nl2_D2_prec16_lr0.001_bs8192_e10", "encode.txt")).read()
                fit = re.findall(r"fit (\S+)s on", log)
                size[codec_name] = sum(int(v) for v in re.findall(r"MSB: (\d+) bytes", log))
                if rep:
                    times.setdefault(codec_name, []).append((te, float(fit[0]) if fit else float("nan")))
        for codec_name, ts in times.items():
            t = [a for a, _ in ts]
            say(f"{name} {side}x{side}x8 {codec_name:8s}: encode.main median {np.median(t):.3f} s, min {min(t):.3f}, max {max(t):.3f} "
                f"(spread {max(t) - min(t):.3f}) | fit {np.median([b for _, b in ts]):.3f} s | MSB payload {size[codec_name]} B = "
                f"{size[codec_name] * 8 / (8 * side * side):.3f} bpsp")
        # the bare call: planes in HBM -> .jp2 bytes on the host, between synchronisations
        planes = ops.to_device_u16(np.ascontiguousarray(img >> 5), "cuda:0")
        ops.jp2k_encode(planes, 16)
        t = []
        for _ in range(repeats + 2):
            torch.cuda.synchronize()
            t0 = time.time()
            b = ops.jp2k_encode(planes, 16)
            t.append(time.time() - t0)
        say(f"{name} {side}x{side}x8 lbdrn_jp2k_encode alone: median {np.median(t):.4f} s, min {min(t):.4f}, max {max(t):.4f}; {len(b)} B")
        old = jp2.set_threads(8)
        x = np.ascontiguousarray(img >> 5)
        t = []
        for _ in range(2):
            t0 = time.time()
            h = jp2.encode(x)
            t.append(time.time() - t0)
        jp2.set_threads(old)
        say(f"{name} {side}x{side}x8 jp2.encode alone (OpenJPEG, 8 threads): min {min(t):.3f} s; {len(h)} B; "
            f"jp2-gpu file is {len(b) - len(h):+d} B against it")
        del planes
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
