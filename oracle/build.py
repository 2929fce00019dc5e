"""Compile oracle/lbdrn_oracle.c, oracle/plane_codec.c and oracle/jp2k_oracle.c into oracle/_build/liblbdrn_oracle.so,
and oracle/jp2k_host_shim.cpp (the product's host-compilable JPEG 2000 text behind a C ABI) into
oracle/_build/libjp2k_host_shim.so.

TEST INFRASTRUCTURE.  Called from __graft_entry__.build() and lazily from
oracle/oracle.py.  -ffp-contract=off keeps gcc from fusing the explicit
mul/add pairs, so every rounding in the C text is the rounding that happens.
-mfma is deliberately not passed: fmaf() goes through glibc, which picks the
hardware FMA at run time when the CPU has one, so the .so also runs (slower,
same bits) on a host without FMA.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "lbdrn_oracle.c"), os.path.join(HERE, "plane_codec.c"), os.path.join(HERE, "jp2k_oracle.c")]
OUT_DIR = os.path.join(HERE, "_build")
OUT = os.path.join(OUT_DIR, "liblbdrn_oracle.so")

CSRC = os.path.join(os.path.dirname(HERE), "lbdrn-msic_amd", "csrc")
SHIM_SRCS = [os.path.join(HERE, "jp2k_host_shim.cpp"), os.path.join(CSRC, "jp2k_t1.inc"), os.path.join(CSRC, "jp2k_t2.inc")]
SHIM_OUT = os.path.join(OUT_DIR, "libjp2k_host_shim.so")


def build(force=False):
    os.makedirs(OUT_DIR, exist_ok=True)
    build_jp2k_host_shim(force)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= max(map(os.path.getmtime, SRCS)):
        return OUT
    cmd = ["gcc", "-O2", "-fPIC", "-shared", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math",
           "-Wall", "-o", OUT] + SRCS + ["-lm"]
    subprocess.check_call(cmd)
    return OUT


def build_jp2k_host_shim(force=False):
    """csrc/jp2k_t1.inc and jp2k_t2.inc compiled by a host C++ compiler; None where there is none (the tests that
    need it then skip and say so; nothing else depends on it)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        return None
    os.makedirs(OUT_DIR, exist_ok=True)
    if not force and os.path.exists(SHIM_OUT) and os.path.getmtime(SHIM_OUT) >= max(map(os.path.getmtime, SHIM_SRCS)):
        return SHIM_OUT
    subprocess.check_call([cxx, "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", SHIM_OUT, SHIM_SRCS[0]])
    return SHIM_OUT


if __name__ == "__main__":
    print(build(force=True))
    print(build_jp2k_host_shim() or "libjp2k_host_shim.so: no C++ compiler, not built")
