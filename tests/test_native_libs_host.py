"""The eight HIP libraries as one table: csrc/build.py's LIBS against the bindings of lbdrn_hip (one _native.Library each),
every binding's table against its header, every built library's exports against its header.  Host only; the libraries
must be built."""
import ctypes
import importlib
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")


def _build_py():
    spec = importlib.util.spec_from_file_location("lbdrn_csrc_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _build_py()
STEMS = [lib["stem"] for lib in B.LIBS]


def binding(stem):
    """the binding module of a library of the build table: the one whose default file name is the table's output"""
    from lbdrn_hip import _native
    for name in _native.BINDINGS:
        mod = importlib.import_module("lbdrn_hip." + name)
        if mod._NATIVE.default == f"liblbdrn_{stem}.so":
            return mod
    pytest.fail(f"no binding of lbdrn_hip._native.BINDINGS loads liblbdrn_{stem}.so")


def built(stem):
    mod = binding(stem)
    if not mod._NATIVE.available():
        pytest.fail(f"liblbdrn_{stem}.so is not built (python lbdrn-msic_amd/csrc/build.py)")
    return mod


RETURNS = {"int": (ctypes.c_int, ctypes.c_int32), "int32_t": (ctypes.c_int, ctypes.c_int32), "size_t": (ctypes.c_size_t,),
           "int64_t": (ctypes.c_int64,), "const char *": (ctypes.c_char_p,)}


def declared(stem):
    """{function: (return type as the header spells it, number of arguments)} of include/<header>, comments stripped"""
    header = next(lib["header"] for lib in B.LIBS if lib["stem"] == stem)
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, args in re.findall(r"(?m)^((?:const\s+)?\w+\s*\*?)\s*\b(lbdrn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        out[name] = (re.sub(r"\s+", " ", ret.strip()), 0 if args.strip() == "void" else args.count(",") + 1)
    assert set(out) == set(re.findall(r"\b(lbdrn_[a-z0-9_]+)\s*\(", text)), "the header has a declaration this parser does not read"
    return out


EXPECTED_DECLARATIONS = {"jp2k_dec": 5, "resid": 8, "tiff": 6, "tiffw": 9, "quality": 5, "pyramid": 7, "plane3": 8}


@pytest.mark.parametrize("stem", STEMS)
def test_binding_table_is_the_header(stem):
    mod = binding(stem)
    decl = declared(stem)
    assert len(decl) == EXPECTED_DECLARATIONS.get(stem, len(decl))
    assert set(decl) == set(mod.SIGNATURES), sorted(set(decl) ^ set(mod.SIGNATURES))
    assert mod._NATIVE.signatures is mod.SIGNATURES and all(n.startswith(mod._NATIVE.prefix) for n in decl)
    for name, (ret, nargs) in decl.items():
        res, args = mod.SIGNATURES[name]
        assert len(args) == nargs, (name, len(args), nargs)
        assert res in RETURNS[ret], (name, ret, res)


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.mark.parametrize("stem", STEMS)
def test_library_exports_exactly_its_header(stem):
    mod = built(stem)
    names, decl = exported(mod._NATIVE.path), set(declared(stem))
    assert names == decl, (sorted(names - decl), sorted(decl - names))


@pytest.mark.parametrize("stem", STEMS)
def test_library_loads_with_the_bindings_abi_version(stem):
    mod = built(stem)
    assert mod.lib() is mod.lib()
    assert getattr(mod.lib(), mod._NATIVE.prefix + "abi_version")() == mod.ABI_VERSION == mod._NATIVE.abi
    header = open(os.path.join(ROOT, "include", next(lib["header"] for lib in B.LIBS if lib["stem"] == stem))).read()
    assert int(re.search(r"#define LBDRN_\w*ABI_VERSION (\d+)", header).group(1)) == mod.ABI_VERSION


def test_build_table_and_bindings_are_one_to_one():
    from lbdrn_hip import _native
    mods = [importlib.import_module("lbdrn_hip." + name) for name in _native.BINDINGS]
    assert [m._NATIVE.default for m in mods] == [os.path.basename(B.output(lib)) for lib in B.LIBS]
    assert len(set(STEMS)) == len(STEMS) == 8 and B.OUT == B.output(B.LIBS[0])
    for m in mods:      # without an override each binding loads what the table builds
        if not os.environ.get(m._NATIVE.env):
            assert m._NATIVE.path == os.path.join(os.path.dirname(CSRC), m._NATIVE.default)
    assert len({m._NATIVE.env for m in mods}) == len({m._NATIVE.prefix for m in mods}) == 8
    for lib in B.LIBS:
        for f in lib["srcs"] + [lib["script"], os.path.join("..", "..", "include", lib["header"])]:
            assert os.path.exists(os.path.join(CSRC, f)), f
    # __graft_entry__.build() loads what this list names
    import __graft_entry__ as entry
    src = inspect.getsource(entry.build)
    assert "for name in _native.BINDINGS" in src and 'import_module("lbdrn_hip." + name).lib()' in src


# What the build script listed by hand, per library, before it read the #include lines (relative to csrc/).  The main
# library had no list (every .hpp and .inc of the directory counted): its sources, the two headers they share, its version
# script and its public header stand for it.
HAND_WRITTEN_DEPS = {
    "hip": ["cabi.hip", "generic.hip", "apply_mfma.hip", "train_mfma.hip", "randperm.hip", "plane_codec.hip", "weights_codec.hip", "jp2k.hip",
            "common.hpp", "lbdrn_math.hpp", "exports.map", "../../include/lbdrn_hip.h"],
    "jp2k_dec": ["jp2k_dec.hip", "jp2k_t1.inc", "jp2k_t2.inc", "jp2k_t1d.inc", "jp2k_t2d.inc", "common.hpp", "exports_jp2k_dec.map",
                 "../../include/lbdrn_hip.h", "../../include/lbdrn_jp2k_dec.h"],
    "resid": ["resid.hip", "resid.inc", "common.hpp", "exports_resid.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_resid.h"],
    "tiff": ["tiff.hip", "tiff.inc", "common.hpp", "exports_tiff.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_tiff.h"],
    "tiffw": ["tiffw.hip", "tiffw.inc", "tiff.inc", "common.hpp", "exports_tiffw.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_tiff.h",
              "../../include/lbdrn_tiff_write.h"],
    "quality": ["quality.hip", "quality.inc", "common.hpp", "exports_quality.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_quality.h"],
    "pyramid": ["pyramid.hip", "pyramid.inc", "common.hpp", "exports_pyramid.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_pyramid.h"],
    "plane3": ["plane3.hip", "plane3.inc", "common.hpp", "exports_plane3.map", "../../include/lbdrn_hip.h", "../../include/lbdrn_plane3.h"],
}


def test_dependency_rule_is_no_narrower_than_the_hand_written_lists():
    assert set(HAND_WRITTEN_DEPS) == set(STEMS)
    for lib in B.LIBS:
        got = B.deps(lib)
        want = {os.path.normpath(os.path.join(CSRC, f)) for f in HAND_WRITTEN_DEPS[lib["stem"]] + ["build.py"]}
        assert all(os.path.isabs(f) and os.path.exists(f) for f in got)
        assert want <= got, (lib["stem"], sorted(want - got))
        # and one library's own text is not another's: the main library does not wait for plane3.inc
        if lib["stem"] != "plane3":
            assert os.path.join(CSRC, "plane3.inc") not in got, lib["stem"]
        # the lane coder and the wave walk are one text for LBB2 (the main library) and LBB3, and nobody else's
        for shared in ("plane_lane.inc", "plane_wave.hpp"):
            assert (os.path.join(CSRC, shared) in got) == (lib["stem"] in ("hip", "plane3")), (lib["stem"], shared)
        includes = [f for f in got if open(f, errors="replace").read().count('#include "error_buffer.inc"')]
        assert len(includes) == 1, (lib["stem"], includes)      # one message buffer per library


def test_each_library_keeps_its_own_error_message():
    resid, plane3 = built("resid"), built("plane3")
    for a, a_info, a_err, b in ((resid, "lbdrn_resid_info", resid.ResidError, plane3), (plane3, "lbdrn_plane3_info", plane3.Plane3Error, resid)):
        before = b._NATIVE.last_error()
        with pytest.raises(a_err) as e:
            a.info(b"")
        assert str(e.value).startswith(a_info + ":") and e.value.status == a.E_ARG
        assert a._NATIVE.last_error() and str(e.value) == f"{a_info}: {a._NATIVE.last_error()}"
        assert b._NATIVE.last_error() == before
    assert plane3._NATIVE.last_error().startswith("lbdrn_plane3_info:") and resid._NATIVE.last_error().startswith("lbdrn_resid_info:")


def test_a_missing_library_file_says_not_built(tmp_path):
    from lbdrn_hip import _native, resid
    gone = str(tmp_path / "liblbdrn_resid.so")
    L = _native.Library(gone, "LBDRN_NO_SUCH_VARIABLE", "lbdrn_resid_", 1, resid.SIGNATURES, resid.ResidError)
    assert L.path == gone and "LBDRN_NO_SUCH_VARIABLE" not in os.environ
    with pytest.raises(resid.ResidError) as e:
        L.lib()
    assert str(e.value) == f"{gone} not built (python lbdrn-msic_amd/csrc/build.py)" and e.value.status is None
    assert L.available() is False


def test_an_abi_version_other_than_the_bindings_is_refused():
    from lbdrn_hip import _native
    resid = built("resid")
    L = _native.Library(resid._PATH, "LBDRN_NO_SUCH_VARIABLE", "lbdrn_resid_", 7, resid.SIGNATURES, resid.ResidError)
    with pytest.raises(resid.ResidError) as e:
        L.lib()
    assert str(e.value) == f"{resid._PATH}: ABI version 1, this binding is for 7"
    assert L.available() is False


def test_the_copies_are_gone():
    """one CDLL call for the HIP libraries, one message buffer, one build function"""
    pkg = os.path.join(ROOT, "lbdrn-msic_amd", "lbdrn_hip")
    loaders = sorted(f for f in os.listdir(pkg) if f.endswith(".py") and "ctypes.CDLL(" in open(os.path.join(pkg, f)).read())
    assert loaders == ["_native.py", "jp2.py"]
    buffers = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".inc", ".hpp")) and
               re.search(r"thread_local char \w+\[512\]", open(os.path.join(CSRC, f)).read())]
    assert buffers == ["error_buffer.inc"]
    text = open(os.path.join(CSRC, "build.py")).read()
    assert not re.search(r"_DEPS\b", text) and set(re.findall(r"^def (build_\w+)", text, re.M)) == {"build_lib", "build_jp2"}
    from lbdrn_hip import _native
    for name in _native.BINDINGS[1:]:      # the satellites share the status constants and keep the names their callers use
        mod = importlib.import_module("lbdrn_hip." + name)
        assert (mod.E_ARG, mod.E_DEVICE, mod.E_UNSUPPORTED, mod.E_WORKSPACE) == (-1, -2, -3, -4)
        assert mod.lib == mod._NATIVE.lib and mod.available == mod._NATIVE.available and mod._PATH == mod._NATIVE.path and callable(mod._check)


def test_the_plane_coders_share_one_text():
    """LBB2 and LBB3 are one lane coder (csrc/plane_lane.inc) and one wave walk (csrc/plane_wave.hpp): the adaptive-k loop, the
    escape code and the ballot's mbcnt stand in one file each, and plane_codec.hip has no coder of its own"""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".inc", ".hpp"))}
    assert [f for f, t in texts.items() if "(N << (kk + 1)) < A" in t] == ["plane_lane.inc"]
    assert [f for f, t in texts.items() if "0x7FFFu << 16" in t] == ["plane_lane.inc"]
    assert [f for f, t in texts.items() if f.startswith("plane") and "mbcnt_hi" in t] == ["plane_wave.hpp"]
    assert sorted(f for f in texts if f.startswith("plane")) == ["plane3.hip", "plane3.inc", "plane_codec.hip", "plane_lane.inc", "plane_wave.hpp"]
    for gone in ("pl_inner", "pl_fold", "LaneCoder"):
        assert gone not in texts["plane_codec.hip"], gone
    assert '#include "plane3.inc"' not in texts["plane_codec.hip"]
