"""Build-time checks on the shipped machine code and its sources.

ADVICE round 3 / VERDICT round 4: the loader wave of k_train_stream used to load its pixel indices with an inline-asm
`global_load_dwordx2` into a register and ride that register through an inline-asm counted wait -- between the two
statements the compiler was free, by the language, to copy or spill a register the hardware had not written yet.  Since
round 5 nothing is loaded into a REGISTER by inline assembly any more: the indices travel by LDS-DMA like the rows and the
fragments (k_train_stream's loader wave, k_train_split), are waited for by a counted `s_waitcnt vmcnt(N)` and read from
LDS by an ordinary load behind it.  These tests keep it that way."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_no_inline_asm_load_writes_a_register():
    """Sources: the only inline-asm memory instructions are LDS-DMA requests (no destination register) and waits."""
    csrc = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".inc", ".hpp")):
            continue
        src = open(os.path.join(csrc, f)).read()
        for m in re.finditer(r'asm\s+volatile\s*\(\s*"([^"]*)"', src):
            text = m.group(1)
            for ins in re.findall(r"(?:global|buffer|flat|scratch)_load_\w+|ds_read\w*|s_load\w*|s_buffer_load\w*", text):
                assert "_lds_" in ins, f"{f}: inline asm `{text[:60]}` loads into a register"


def test_loader_waits_for_its_indices_behind_a_counted_wait(tmp_path):
    """Machine code: in every k_train_stream instance the first vector-memory instruction of the loader's path is an LDS-DMA
    request (the indices), nothing is loaded to a register before the first counted wait, and that wait allows no more
    requests in flight than were issued behind the first one (requests complete in order: the indices have landed)."""
    so = os.path.join(ROOT, "lbdrn-msic_amd", "liblbdrn_hip.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(so)):
        pytest.skip("llvm-objdump or the library is missing")
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(so, work / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)   # unbundles next to the input
    checked = 0
    for co in sorted(work.glob("lib.so.*gfx950")):
        syms = subprocess.run([OBJDUMP, "-t", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "k_train_stream" in l and " F " in l and l.split()[-1].startswith("_Z")})
        for name in names:
            dis = subprocess.run([OBJDUMP, "-d", f"--disassemble-symbols={name}", str(co)], capture_output=True, text=True).stdout
            lines = [l.split("//")[0].strip() for l in dis.splitlines() if l.startswith("\t")]
            dma = [k for k, l in enumerate(lines) if l.startswith("global_load_lds_dwordx4")]
            assert dma, f"{name}: no LDS-DMA request found"
            behind = 0
            for l in lines[dma[0] + 1:]:
                if l.startswith("s_waitcnt") and "vmcnt" in l:
                    n = int(re.search(r"vmcnt\((\d+)\)", l).group(1))
                    assert n <= behind, f"{name}: the wait for the indices allows {n} requests in flight, only {behind} were issued behind them"
                    break
                assert not re.match(r"(global|buffer|flat)_load_(dword|ubyte|ushort|sbyte|sshort)", l) or "_lds_" in l, \
                    f"{name}: `{l}` loads a register between the index request and its wait"
                behind += l.startswith("global_load_lds_dwordx4")
                assert not l.startswith("s_endpgm"), f"{name}: no vector-memory wait behind the index request"
            checked += 1
    assert checked >= 4, "k_train_stream instances not found in the library's code objects"


def test_shipped_library_exports_the_c_abi_only_and_no_kernel_uses_scratch():
    """the library is a product -- `nm -D` shows the functions of include/lbdrn_hip.h and no C++ symbol
    (-fvisibility=hidden + csrc/exports.map), no kernel in it spills (k_apply_mfma<4, 2> did: 88 registers), and its
    sources read no environment variable (every build switch is a -D of csrc/build.py --variant)."""
    import sys
    so = os.path.join(ROOT, "lbdrn-msic_amd", "liblbdrn_hip.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(so)):
        pytest.skip("llvm-objdump or the library is missing")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert names and all(n.startswith("lbdrn_") for n in names), [n for n in names if not n.startswith("lbdrn_")][:5]
    header = open(os.path.join(ROOT, "include", "lbdrn_hip.h")).read()
    declared = set(re.findall(r"\b(lbdrn_[a-z0-9_]+)\s*\(", header))
    assert set(names) == declared, (sorted(set(names) - declared), sorted(declared - set(names)))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    rows = kernel_resources(so)
    assert len(rows) > 50
    bad = [(r["demangled"], r["spill_vgpr"], r["scratch"]) for r in rows if r["spill_vgpr"] or r["scratch"]]
    assert not bad, bad
    csrc = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".inc", ".hpp", ".c")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_nothing_of_the_dropped_overlap_experiment_ships():
    """Round 5's "next training launch beside the reduce launch" experiment (scripts/experiments/reduce_beside_next_launch.patch)
    ended in a SIGABRT from the runtime whose cause was never established.  None of its mechanisms is in the
    library: no launch through hipExtLaunchKernelGGL / hipExtAnyOrderLaunch, no kernel that waits in a loop for another
    launch's store (s_sleep / a polling atomic load), no release / acquire fence between launches, no sync words in the
    training workspace.  A launch of this library depends on its predecessors through stream order only."""
    csrc = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".inc", ".hpp")):
            continue
        src = open(os.path.join(csrc, f)).read()
        for word in ("hip_ext.h", "hipExtLaunchKernelGGL", "hipExtAnyOrderLaunch", "s_sleep", "off_sync",
                     "hipStreamWaitEvent", "hipEventRecord"):
            assert word not in src, f"{f}: {word}"
        # (fences of wavefront scope order a wave's own LDS traffic -- randperm.hip --; what the experiment had were fences of
        #  agent scope between two launches)
        for m in re.finditer(r"__builtin_amdgcn_fence\(([^)]*)\)", src):
            assert '"agent"' not in m.group(1) and '"system"' not in m.group(1) and m.group(1).strip().endswith('"wavefront"'), f"{f}: {m.group(0)}"


def test_the_only_build_switches_are_the_measurement_instruments():
    """The A/B alternatives, timing-only arms and fixed numeric tunables of rounds 1-6 were removed from csrc/ (DESIGN 1,
    "Build switches"; they last exist in commit ac69733).  What is left to switch at build time are the four instruments:
    the in-kernel phase stamps and the per-step timeline.  Every LBDRN_ macro an #if / #ifdef / #ifndef / #elif line of the
    sources tests, inside defined(...) too, is one of them: a new measurement switch is added to this list on purpose."""
    instruments = {"LBDRN_TRAIN_STAMPS", "LBDRN_APPLY_STAMPS", "LBDRN_STAMP_DW", "LBDRN_TIMELINE"}
    csrc = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
    seen = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".inc", ".hpp")):
            continue
        src = open(os.path.join(csrc, f)).read().replace("\\\n", " ")   # (continued directive lines as one)
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif|elifdef|elifndef)\b(.*)$", src, re.M):
            names = set(re.findall(r"\bLBDRN_[A-Z0-9_]+", m.group(1).split("//")[0]))
            assert names <= instruments, f"{f}: {m.group(0).strip()[:80]} tests {sorted(names - instruments)}"
            seen |= names
    assert seen == instruments, sorted(instruments - seen)


def test_the_training_kernels_in_the_library_are_exactly_the_listed_instances(tmp_path):
    """Kernel symbols only: the k_train_stream<..>, k_train_split<..> and k_train_mfma<..> instances in the shipped library's
    gfx950 code object are the ones the three lists of csrc/train_mfma.hip name (tests/train_plan_reference.py:
    built_instances) -- nothing that no shape reaches is compiled, nothing a shape reaches is missing."""
    import sys
    so = os.path.join(ROOT, "lbdrn-msic_amd", "liblbdrn_hip.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(so)):
        pytest.skip("llvm-objdump or the library is missing")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train_plan_reference as R
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(so, work / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)   # unbundles next to the input
    found = set()
    for co in sorted(work.glob("lib.so.*gfx950")):
        syms = subprocess.run([OBJDUMP, "--syms", "-C", str(co)], capture_output=True, text=True, check=True).stdout
        for kernel, args in re.findall(r"\blbdrn::k_train_(stream|split|mfma)<([\d, ]+)>\(", syms):
            a = [int(x) for x in args.split(",")]
            if kernel == "stream":      # <LQ, NL, PD, NT0C, ACT>
                found.add(("stream", a[0], a[1], a[3], R.ACTS[a[4]]))
            elif kernel == "split":     # <LQ, NT0C, ACT>
                found.add(("split", a[0], 2, a[1], R.ACTS[a[2]]))
            else:                       # <LQ, NL>
                found.add(("tile", a[0], a[1], 0, "sine"))
    built = set(R.built_instances())
    assert found == built, (sorted(found - built), sorted(built - found))


def test_the_apply_kernels_in_the_library_are_exactly_the_listed_instances(tmp_path):
    """Kernel symbols only, the twin of the test above for the fused apply pass: the k_apply_mfma<NT, MODE, RELU> and
    k_apply_wide<NT, NL, MODE> instances in the shipped library's gfx950 code object are the ones APPLY_INSTANCES (each row for
    Sine and ReLU) and WAPPLY_INSTANCES (each row in the decode, the canonical and the fast evaluation mode) of
    csrc/apply_mfma.hip name: 20 and 12."""
    so = os.path.join(ROOT, "lbdrn-msic_amd", "liblbdrn_hip.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(so)):
        pytest.skip("llvm-objdump or the library is missing")
    src = open(os.path.join(ROOT, "lbdrn-msic_amd", "csrc", "apply_mfma.hip")).read()
    modes = {name: int(v) for name, v in re.findall(r"\b(MODE_[A-Z0-9_]+) = (\d+)", src)}
    assert modes == {"MODE_DECODE": 0, "MODE_EVAL": 1, "MODE_EVAL_FAST": 2, "MODE_EVAL_X16": 3}
    rows = [(int(nt), modes[m]) for nt, m in re.findall(r"\bX\((\d+), (MODE_[A-Z0-9_]+)\)", src)]
    wrows = [(int(nt), int(nl)) for nt, nl in re.findall(r"\bX\((\d+), (\d+)\)", src)]
    listed = {("mfma", nt, m, relu) for nt, m in rows for relu in ("false", "true")} | \
             {("wide", nt, nl, m) for nt, nl in wrows for m in (modes["MODE_DECODE"], modes["MODE_EVAL"], modes["MODE_EVAL_FAST"])}
    assert len(rows) == len(set(rows)) == 10 and len(wrows) == len(set(wrows)) == 4 and len(listed) == 32
    work = tmp_path / "co"
    work.mkdir()
    shutil.copy(so, work / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, check=True, capture_output=True)   # unbundles next to the input
    found = set()
    for co in sorted(work.glob("lib.so.*gfx950")):
        syms = subprocess.run([OBJDUMP, "--syms", "-C", str(co)], capture_output=True, text=True, check=True).stdout
        for nt, m, relu in re.findall(r"\blbdrn::k_apply_mfma<(\d+), (\d+), (true|false)>\(", syms):
            found.add(("mfma", int(nt), int(m), relu))
        for nt, nl, m in re.findall(r"\blbdrn::k_apply_wide<(\d+), (\d+), (\d+)>\(", syms):
            found.add(("wide", int(nt), int(nl), int(m)))
    assert found == listed, (sorted(found - listed), sorted(listed - found))
