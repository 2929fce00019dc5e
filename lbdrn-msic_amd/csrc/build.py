"""Build liblbdrn_hip.so, liblbdrn_jp2k_dec.so, liblbdrn_resid.so, liblbdrn_tiff.so, liblbdrn_tiffw.so, liblbdrn_quality.so, liblbdrn_pyramid.so and liblbdrn_plane3.so for gfx950 with hipcc (in-tree, next to the Python host code).

    python lbdrn-msic_amd/csrc/build.py [--force]

-ffp-contract=off: the canonical arithmetic (lbdrn_math.hpp) spells out every fma; the compiler
must not invent more.  -fhip-fp32-correctly-rounded-divide-sqrt: IEEE division for the
normalisation p = msb/max and the sigmoid (the reference divides in numpy / torch float32).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = ["cabi.hip", "generic.hip", "apply_mfma.hip", "train_mfma.hip", "randperm.hip", "plane_codec.hip", "weights_codec.hip", "jp2k.hip"]
HDRS = sorted(f for f in os.listdir(HERE) if f.endswith((".hpp", ".inc"))) + ["exports.map", "../../include/lbdrn_hip.h"]
OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-fvisibility=hidden"]   # the exports are the functions include/lbdrn_hip.h declares, nothing else


JP2_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_jp2.so")


def build_jp2(force=False):
    """liblbdrn_jp2.so (include/lbdrn_jp2.h): OpenJPEG behind a C ABI, gcc, host only.  Built where openjpeg.h and
    libopenjp2 are found (this image: /opt/conda); returns None elsewhere -- the JPEG 2000 payload is then unavailable
    and says so, the default GPU payload does not need it."""
    import glob
    src = os.path.join(HERE, "jp2_shim.c")
    hdr = os.path.join(HERE, "..", "..", "include", "lbdrn_jp2.h")
    if not force and os.path.exists(JP2_OUT) and os.path.getmtime(JP2_OUT) > max(os.path.getmtime(src), os.path.getmtime(hdr)):
        return JP2_OUT
    for root in ("/opt/conda", "/usr", "/usr/local"):
        incs = sorted(glob.glob(os.path.join(root, "include", "openjpeg-*", "openjpeg.h")))
        libs = [d for d in (os.path.join(root, "lib"), os.path.join(root, "lib", "x86_64-linux-gnu"))
                if glob.glob(os.path.join(d, "libopenjp2.so*"))]
        if incs and libs:
            lib = sorted(glob.glob(os.path.join(libs[0], "libopenjp2.so*")))[0]
            cmd = [os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-Wall", "-fvisibility=hidden", "-I" + os.path.dirname(incs[-1]), "-o", JP2_OUT, src,
                   lib, "-Wl,-rpath," + libs[0]]
            subprocess.check_call(cmd)
            return JP2_OUT
    return None


JP2K_DEC_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_jp2k_dec.so")
JP2K_DEC_SRCS = ["jp2k_dec.hip"]
JP2K_DEC_DEPS = ["jp2k_t1.inc", "jp2k_t2.inc", "jp2k_t1d.inc", "jp2k_t2d.inc", "common.hpp", "exports_jp2k_dec.map",
                 "../../include/lbdrn_hip.h", "../../include/lbdrn_jp2k_dec.h"]


def build_jp2k_dec(force=False):
    """liblbdrn_jp2k_dec.so (include/lbdrn_jp2k_dec.h): the GPU decoder of the JPEG 2000 payload, a library of its own
    beside liblbdrn_hip.so -- same compiler, same flags, its own object files and version script."""
    if not force and os.path.exists(JP2K_DEC_OUT):
        t = os.path.getmtime(JP2K_DEC_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in JP2K_DEC_SRCS + JP2K_DEC_DEPS + ["build.py"]):
            return JP2K_DEC_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in JP2K_DEC_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_jp2k_dec.map"), "-o", JP2K_DEC_OUT] + objs)
    return JP2K_DEC_OUT


RESID_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_resid.so")
RESID_SRCS = ["resid.hip"]
RESID_DEPS = ["resid.inc", "common.hpp", "exports_resid.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_resid.h"]


def build_resid(force=False):
    """liblbdrn_resid.so (include/lbdrn_resid.h): the residual layer's coder and decoder, a library of its own like
    liblbdrn_jp2k_dec.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(RESID_OUT):
        t = os.path.getmtime(RESID_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in RESID_SRCS + RESID_DEPS + ["build.py"]):
            return RESID_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in RESID_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_resid.map"), "-o", RESID_OUT] + objs)
    return RESID_OUT


TIFF_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_tiff.so")
TIFF_SRCS = ["tiff.hip"]
TIFF_DEPS = ["tiff.inc", "common.hpp", "exports_tiff.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_tiff.h"]


def build_tiff(force=False):
    """liblbdrn_tiff.so (include/lbdrn_tiff.h): the TIFF reader's segment decoders and placement, a library of its own
    like liblbdrn_resid.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(TIFF_OUT):
        t = os.path.getmtime(TIFF_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in TIFF_SRCS + TIFF_DEPS + ["build.py"]):
            return TIFF_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in TIFF_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_tiff.map"), "-o", TIFF_OUT] + objs)
    return TIFF_OUT


TIFFW_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_tiffw.so")
TIFFW_SRCS = ["tiffw.hip"]
TIFFW_DEPS = ["tiffw.inc", "tiff.inc", "common.hpp", "exports_tiffw.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_tiff.h",
              "../../include/lbdrn_tiff_write.h"]


def build_tiffw(force=False):
    """liblbdrn_tiffw.so (include/lbdrn_tiff_write.h): the TIFF writer's gather, Deflate encoder and packing, a library of
    its own like liblbdrn_tiff.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(TIFFW_OUT):
        t = os.path.getmtime(TIFFW_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in TIFFW_SRCS + TIFFW_DEPS + ["build.py"]):
            return TIFFW_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in TIFFW_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_tiffw.map"), "-o", TIFFW_OUT] + objs)
    return TIFFW_OUT


QUALITY_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_quality.so")
QUALITY_SRCS = ["quality.hip"]
QUALITY_DEPS = ["quality.inc", "common.hpp", "exports_quality.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_quality.h"]


def build_quality(force=False):
    """liblbdrn_quality.so (include/lbdrn_quality.h): the comparison of two rasters in HBM -- error statistics, SSIM and SAM --
    a library of its own like liblbdrn_tiffw.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(QUALITY_OUT):
        t = os.path.getmtime(QUALITY_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in QUALITY_SRCS + QUALITY_DEPS + ["build.py"]):
            return QUALITY_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in QUALITY_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_quality.map"), "-o", QUALITY_OUT] + objs)
    return QUALITY_OUT


PYRAMID_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_pyramid.so")
PYRAMID_SRCS = ["pyramid.hip"]
PYRAMID_DEPS = ["pyramid.inc", "common.hpp", "exports_pyramid.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_pyramid.h"]


def build_pyramid(force=False):
    """liblbdrn_pyramid.so (include/lbdrn_pyramid.h): the overview levels of a raster in HBM, a library of its own like
    liblbdrn_quality.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(PYRAMID_OUT):
        t = os.path.getmtime(PYRAMID_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in PYRAMID_SRCS + PYRAMID_DEPS + ["build.py"]):
            return PYRAMID_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in PYRAMID_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_pyramid.map"), "-o", PYRAMID_OUT] + objs)
    return PYRAMID_OUT


PLANE3_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_plane3.so")
PLANE3_SRCS = ["plane3.hip"]
PLANE3_DEPS = ["plane3.inc", "common.hpp", "exports_plane3.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_plane3.h"]


def build_plane3(force=False):
    """liblbdrn_plane3.so (include/lbdrn_plane3.h): the LBB3 coder and decoder of the MSB payload, a library of its own like
    liblbdrn_pyramid.so -- same compiler, same flags, its own object file and version script."""
    if not force and os.path.exists(PLANE3_OUT):
        t = os.path.getmtime(PLANE3_OUT)
        if not any(os.path.getmtime(os.path.join(HERE, f)) > t for f in PLANE3_SRCS + PLANE3_DEPS + ["build.py"]):
            return PLANE3_OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in PLANE3_SRCS:
        obj = os.path.join(HERE, src.replace(".hip", ".o"))
        objs.append(obj)
        subprocess.check_call([hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + ["-o", obj, os.path.join(HERE, src)])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
                           "-Wl,--version-script=" + os.path.join(HERE, "exports_plane3.map"), "-o", PLANE3_OUT] + objs)
    return PLANE3_OUT


def stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SRCS + HDRS + ["build.py"])


def build(force=False, extra=(), out=None):
    out = out or OUT
    if out == OUT:
        build_jp2k_dec(force)
        build_resid(force)
        build_tiff(force)
        build_tiffw(force)
        build_quality(force)
        build_pyramid(force)
        build_plane3(force)
    if out == OUT and not force and not stale():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    for src in SRCS:
        tag = "" if out == OUT else "." + os.path.basename(out)[len("liblbdrn_hip_"):-len(".so")]   # objects per variant
        obj = os.path.join(HERE, src.replace(".hip", tag + ".o"))
        objs.append(obj)
        cmd = [hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + list(extra) + \
              ["-o", obj, os.path.join(HERE, src)]
        procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(HERE, "exports.map"),
                           "-o", out] + objs)
    return out


if __name__ == "__main__":
    if "--stamps" in sys.argv:  # diagnostic build with in-kernel s_memtime stamps (never benchmarked)
        print(build(force=True, extra=["-DLBDRN_TRAIN_STAMPS", "-DLBDRN_APPLY_STAMPS"],
                    out=os.path.join(os.path.dirname(HERE), "liblbdrn_hip_stamps.so")))
    elif "--variant" in sys.argv:  # A/B build: python build.py --variant NAME -DFOO ... -> liblbdrn_hip_NAME.so
        k = sys.argv.index("--variant")
        print(build(force=True, extra=[a for a in sys.argv[k + 2:] if a.startswith("-D")],
                    out=os.path.join(os.path.dirname(HERE), f"liblbdrn_hip_{sys.argv[k + 1]}.so")))
    else:
        print(build(force="--force" in sys.argv))
        print(JP2K_DEC_OUT)
        print(RESID_OUT)
        print(TIFF_OUT)
        print(TIFFW_OUT)
        print(QUALITY_OUT)
        print(PYRAMID_OUT)
        print(PLANE3_OUT)
        print(build_jp2(force="--force" in sys.argv) or "liblbdrn_jp2.so: OpenJPEG not found, not built")
