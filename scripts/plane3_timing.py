"""LBB3 (the MSB payload with inter-band prediction, csrc/plane3.hip) beside LBB2 and the GPU JPEG 2000 coder: rate and time.

    python scripts/plane3_timing.py --rate [--out profiles/plane3_rate.txt]
        no GPU: the sequential restatement's byte count (tests/plane3_reference.py) against the LBB2 restatement's on the
        256 x 256 tiles the host tests assert on.
    python scripts/plane3_timing.py [--repeats N] [--out profiles/plane3_timing.txt]
        on the GPU, in one process: lbdrn_plane_encode / _decode (LBB2), lbdrn_plane3_encode / _decode and lbdrn_jp2k_encode
        between HIP events, buffers allocated beforehand, on synthetic_tile(0) (independent bands) and correlated_tile(0)
        (bands that share their structure) at 8 x 2048^2 and 4 x 2048^2, K = 3, 5, 7; one warm-up and N counted runs each;
        the bpsp of each; then encode.main file to file under LBB2, LBB3 and jp2-gpu, alternating."""
import ctypes
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np

from lbdrn_hip.synth import correlated_tile, synthetic_tile

argv = sys.argv[1:]
repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish():
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if "--rate" in argv:
    import oracle as O
    import plane3_reference as R
    say("LBB3 against LBB2, both by their sequential restatements (bytes of the body, tag and frame excluded), 256 x 256 tiles")
    for name, x in ([(f"correlated_tile(0, {C}, 256, 256) >> 5", correlated_tile(0, C, 256, 256) >> 5) for C in (8, 4)] +
                    [(f"synthetic_tile(0, 8, 256, 256) >> {K}", synthetic_tile(0, 8, 256, 256) >> K) for K in (3, 5, 7)]):
        counts, words = O.plane_encode(np.ascontiguousarray(x, np.uint16))
        n2, n3 = 4 * (counts.size + words.size), len(R.encode(x))
        say(f"   {name:40s} LBB2 {n2:7d} B = {8 * n2 / x.size:.3f} bpsp | LBB3 {n3:7d} B = {8 * n3 / x.size:.3f} bpsp | LBB3 / LBB2 = {n3 / n2:.4f} "
            f"({100 * (n3 / n2 - 1):+.2f} %)")
    finish()
    sys.exit(0)

import torch

import encode
from lbdrn_hip import _lib, ops, plane3, raster_io

dev = torch.device("cuda:0")
L2, L3 = _lib.lib(), plane3.lib()
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
vp = ctypes.c_void_p


def timed(fn):
    """one warm-up, then `repeats` runs between HIP events -> seconds"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e-3)
    return t


def fmt(t):
    return f"min {min(t) * 1e3:8.3f} median {np.median(t) * 1e3:8.3f} max {max(t) * 1e3:8.3f} ms"


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: status {rc}")


say(f"== events: device {torch.cuda.get_device_name(0)}; planes in HBM, buffers allocated beforehand; 1 warm-up + {repeats} runs of each call")
scenes = {"synthetic_tile(0)": synthetic_tile(0, 8, 2048, 2048), "correlated_tile(0)": correlated_tile(0, 8, 2048, 2048)}
for scene, img in scenes.items():
    for C in (8, 4):
        for K in (3, 5, 7):
            x = np.ascontiguousarray(img[:C] >> K)
            H, W = x.shape[1:]
            planes = ops.to_device_u16(x, dev)
            back = torch.empty_like(planes)
            nbytes = torch.zeros(1, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            say(f"   {scene} >> {K}, {C} x {H} x {W}")
            # LBB2
            cap, nws = L2.lbdrn_plane_bound(C, H, W), L2.lbdrn_plane_workspace(C, H, W)
            body, ws = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(nws, dtype=torch.uint8, device=dev)
            t = timed(lambda: ok(L2.lbdrn_plane_encode(vp(planes.data_ptr()), C, H, W, vp(body.data_ptr()), cap, vp(nbytes.data_ptr()), vp(ws.data_ptr()), nws, stream), "lbdrn_plane_encode"))
            n2 = int(nbytes.item())
            say(f"      lbdrn_plane_encode  (LBB2)   {fmt(t)} | {n2:9d} B = {8 * n2 / x.size:.3f} bpsp")
            t = timed(lambda: ok(L2.lbdrn_plane_decode(vp(body.data_ptr()), n2, C, H, W, vp(back.data_ptr()), vp(status.data_ptr()), vp(ws.data_ptr()), nws, stream), "lbdrn_plane_decode"))
            assert int(status.item()) == 0 and torch.equal(back, planes)
            say(f"      lbdrn_plane_decode  (LBB2)   {fmt(t)}")
            del body, ws
            # LBB3
            cap, nws, dws = L3.lbdrn_plane3_bound(C, H, W), L3.lbdrn_plane3_encode_workspace(C, H, W), L3.lbdrn_plane3_decode_workspace(C, H, W)
            body, ws = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(nws, dtype=torch.uint8, device=dev)
            t = timed(lambda: ok(L3.lbdrn_plane3_encode(planes.data_ptr(), C, H, W, body.data_ptr(), cap, nbytes.data_ptr(), ws.data_ptr(), nws, stream), "lbdrn_plane3_encode"))
            n3 = int(nbytes.item())
            say(f"      lbdrn_plane3_encode (LBB3)   {fmt(t)} | {n3:9d} B = {8 * n3 / x.size:.3f} bpsp | LBB3 / LBB2 = {n3 / n2:.4f}")
            back.zero_()
            t = timed(lambda: ok(L3.lbdrn_plane3_decode(body.data_ptr(), n3, C, H, W, 256, back.data_ptr(), status.data_ptr(), ws.data_ptr(), dws, stream), "lbdrn_plane3_decode"))
            assert int(status.item()) == 0 and torch.equal(back, planes)
            say(f"      lbdrn_plane3_decode (LBB3)   {fmt(t)}")
            del body, ws
            # JPEG 2000 on the GPU (the call ends with the file in host memory)
            out = np.empty(L2.lbdrn_jp2k_bound(C, H, W), np.uint8)
            size = {}
            t = timed(lambda: size.__setitem__("n", len(ops.jp2k_encode(planes, 16, out=out))))
            say(f"      lbdrn_jp2k_encode   (jp2-gpu) {fmt(t)} | {size['n']:9d} B = {8 * size['n'] / x.size:.3f} bpsp")
            del planes, back, out

say(f"== wall: encode.main file to file, K = 5, default arguments; 1 warm-up + {repeats} runs of each codec, alternating")
with tempfile.TemporaryDirectory() as d:
    for scene, img in scenes.items():
        name = scene.split("(")[0]
        src = os.path.join(d, f"{name}.npy")
        raster_io.write_raster(src, img)
        times, size = {}, {}
        for rep in range(repeats + 1):
            for codec_name in ("LBB2", "LBB3", "jp2-gpu"):
                encode.BASE_CODEC = codec_name
                out = os.path.join(d, f"o_{name}_{codec_name}_{rep}")
                torch.cuda.synchronize()
                t0 = time.time()
                encode.main(["-i", src, "-o", out])
                te = time.time() - t0
                (sub,) = os.listdir(out)
                log = open(os.path.join(out, sub, "encode.txt")).read()
                size[codec_name] = sum(int(v) for v in re.findall(r"MSB: (\d+) bytes", log))
                if rep:
                    times.setdefault(codec_name, []).append(te)
        for codec_name, t in times.items():
            say(f"   {scene} 8 x 2048 x 2048 {codec_name:8s}: encode.main median {np.median(t):.3f} s, min {min(t):.3f}, max {max(t):.3f} | "
                f"MSB payload {size[codec_name]} B = {size[codec_name] * 8 / img.size:.3f} bpsp")
    encode.BASE_CODEC = "LBB2"
finish()
