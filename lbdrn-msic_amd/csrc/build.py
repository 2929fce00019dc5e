"""Build the HIP libraries of LIBS -- liblbdrn_hip.so and the libraries beside it -- for gfx950 with hipcc (in-tree, next
to the Python host code), and the optional OpenJPEG shim liblbdrn_jp2.so with gcc.

    python lbdrn-msic_amd/csrc/build.py [--force]

-ffp-contract=off: the canonical arithmetic (lbdrn_math.hpp) spells out every fma; the compiler
must not invent more.  -fhip-fp32-correctly-rounded-divide-sqrt: IEEE division for the
normalisation p = msb/max and the sigmoid (the reference divides in numpy / torch float32).
"""
import os
import re
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-fvisibility=hidden"]   # the exports are the functions the library's header declares, nothing else

# One entry per HIP library: liblbdrn_<stem>.so is linked from the objects of `srcs` with the version script `script` and
# exports what include/<header> declares.  Every library has the same compiler and flags and its own object files.  The
# first entry is the main library; it alone takes build()'s `extra` flags and `out` override.
LIBS = [
    dict(stem="hip", header="lbdrn_hip.h", script="exports.map",
         srcs=["cabi.hip", "generic.hip", "apply_mfma.hip", "train_mfma.hip", "randperm.hip", "plane_codec.hip", "weights_codec.hip",
               "jp2k.hip"]),
    dict(stem="jp2k_dec", header="lbdrn_jp2k_dec.h", script="exports_jp2k_dec.map", srcs=["jp2k_dec.hip"]),   # JPEG 2000 decoder
    dict(stem="resid", header="lbdrn_resid.h", script="exports_resid.map", srcs=["resid.hip"]),               # residual layer
    dict(stem="tiff", header="lbdrn_tiff.h", script="exports_tiff.map", srcs=["tiff.hip"]),                   # TIFF reader
    dict(stem="tiffw", header="lbdrn_tiff_write.h", script="exports_tiffw.map", srcs=["tiffw.hip"]),          # TIFF writer
    dict(stem="quality", header="lbdrn_quality.h", script="exports_quality.map", srcs=["quality.hip"]),       # quality report
    dict(stem="pyramid", header="lbdrn_pyramid.h", script="exports_pyramid.map", srcs=["pyramid.hip"]),       # overview levels
    dict(stem="plane3", header="lbdrn_plane3.h", script="exports_plane3.map", srcs=["plane3.hip"]),           # LBB3 MSB payload
]


def output(lib):
    return os.path.join(os.path.dirname(HERE), f"liblbdrn_{lib['stem']}.so")


OUT = output(LIBS[0])
JP2_OUT = os.path.join(os.path.dirname(HERE), "liblbdrn_jp2.so")
_COMPILERS = threading.BoundedSemaphore(16)   # compiler processes at once, however many libraries the table has


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


def deps(lib):
    """The files a library is built from: its sources, everything they reach through #include "..." lines (resolved beside
    the including file; <...> includes belong to the toolchain), its version script and this file."""
    found, todo = set(), [os.path.join(HERE, f) for f in lib["srcs"]]
    while todo:
        path = os.path.normpath(todo.pop())
        if path not in found:
            found.add(path)
            with open(path) as f:
                todo += [os.path.join(os.path.dirname(path), inc) for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read(), re.M)]
    return found | {os.path.join(HERE, lib["script"]), os.path.join(HERE, "build.py")}


def _stale(lib, out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in deps(lib))


def stale():
    return _stale(LIBS[0], OUT)


def _run(cmd):
    with _COMPILERS:
        subprocess.check_call(cmd)


def build_lib(lib, force=False, extra=(), out=None):
    """One entry of LIBS: nothing if `out` is newer than deps(lib), else its sources compiled side by side and linked."""
    out = out or output(lib)
    tag = "" if out == output(lib) else "." + os.path.basename(out)[len(f"liblbdrn_{lib['stem']}_"):-len(".so")]   # objects per variant
    if not force and not _stale(lib, out):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [os.path.join(HERE, src.replace(".hip", tag + ".o")) for src in lib["srcs"]]
    with ThreadPoolExecutor(len(objs)) as pool:
        list(pool.map(_run, [[hipcc, "-c"] + [f for f in FLAGS if f != "-shared"] + list(extra) + ["-o", obj, os.path.join(HERE, src)]
                             for src, obj in zip(lib["srcs"], objs)]))
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(HERE, lib["script"]), "-o", out] + objs)
    return out


def build(force=False, extra=(), out=None):
    """Every library of LIBS, side by side; or, with `out`, that variant of the main library alone (always rebuilt)."""
    if out and out != OUT:
        return build_lib(LIBS[0], True, extra, out)
    with ThreadPoolExecutor(len(LIBS)) as pool:
        return list(pool.map(lambda lib: build_lib(lib, force, extra if lib is LIBS[0] else ()), LIBS))[0]


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
        for lib in LIBS[1:]:
            print(output(lib))
        print(build_jp2(force="--force" in sys.argv) or "liblbdrn_jp2.so: OpenJPEG not found, not built")
