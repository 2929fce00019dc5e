"""The C ABI as a caller that is not lbdrn_hip/ops.py meets it, on a machine with no device: what include/lbdrn_hip.h says
about pointer alignment, a NULL msb and large minibatch sizes is checked on the host, in front of the device probe, so
every refusal here comes from the real entry point with pointer VALUES that are never dereferenced.

  * one refusal per declared alignment (lbdrn_hip.h, "Alignment"): the call with every pointer at its declared alignment
    gets past the argument checks (LBDRN_E_DEVICE here, 0 on a GPU machine never happens: the pointers are not memory);
    the same call with ONE pointer moved off its alignment answers LBDRN_E_ARG and names that argument.  The offset is
    one element where that breaks the alignment (4 bytes off a 16-byte `params`, 4 off a 256-byte workspace, 1 off the
    byte-typed LBB2 body) and half the alignment where the alignment IS the element (1 byte off a uint16 plane, 2 off a
    float array, 4 off an int64 array);
  * the NULL-msb rule of lbdrn_eval_sse;
  * lbdrn_train_workspace up to INT32_MAX rows: size_t arithmetic, no wrap.

The libraries must be built (the loader idiom of tests/test_native_libs_host.py)."""
import ctypes
import re

import numpy as np
import pytest

from lbdrn_hip import _lib, _native

E_ARG, E_DEVICE = _native.E_ARG, _native.E_DEVICE
BASE = 0x7F0000000000          # a 4 KiB-aligned address nobody maps: the checks read the value, never the memory


def L():
    if not _lib._NATIVE.available():
        pytest.fail("liblbdrn_hip.so is not built (python lbdrn-msic_amd/csrc/build.py)")
    return _lib.lib()


def no_device():
    return L().lbdrn_device_check() != 0


def last_error():
    return (L().lbdrn_last_error() or b"").decode()


class P:
    """a pointer argument of a call: its name in the header, its declared alignment and element size"""

    def __init__(self, name, align, elem, slot):
        self.name, self.align, self.elem, self.slot = name, align, elem, slot

    def value(self, off=0):
        return ctypes.c_void_p(BASE + 4096 * (self.slot + 1) + off)

    def misplaced(self):
        """off by one element where that leaves the declared alignment, else by half the alignment"""
        off = self.elem if self.elem % self.align else self.align // 2
        assert 0 < off < self.align and (BASE + off) % self.align
        return off


def ptrs(*spec):
    return [P(name, align, elem, k) for k, (name, align, elem) in enumerate(spec)]


U16, F32, I32, I64, F64, WS = 2, 4, 4, 8, 8, 256
TABLES = (ctypes.c_float * 64)()


def geom(C=3, H=9, W=12, K=5, D=2, P_=0, rowtab=None, coltab=None):
    return _lib.Geom(C, H, W, K, D, 100, 1, 1, P_, 0, rowtab, coltab)


def net_of(g, bc=64, nl=2, act=0):
    F = 2 * g.P + g.C * (2 * g.D + 1) ** 2
    return _lib.Net(F, bc, g.C, nl, act)


G = geom()
NET = net_of(G)
BIG = 1 << 40                  # a workspace size no sizing function exceeds here (the size check follows the device probe anyway)
byref = ctypes.byref

# entry point -> (pointer arguments, call(values: name -> c_void_p) -> status)
CALLS = {}


def entry(name, *spec):
    def deco(fn):
        CALLS[name] = (ptrs(*spec), fn)
        return fn
    return deco


@entry("lbdrn_split_bits", ("img", 2, U16), ("msb", 2, U16), ("msb_max", 4, I32))
def _(v):
    return L().lbdrn_split_bits(v["img"], 3, 9, 12, 5, v["msb"], v["msb_max"], None)


@entry("lbdrn_labels", ("img", 2, U16), ("idx", 8, I64), ("labels", 4, F32))
def _(v):
    return L().lbdrn_labels(v["img"], 3, 9, 12, 5, v["idx"], 50, v["labels"], None)


@entry("lbdrn_features", ("msb", 2, U16), ("idx", 8, I64), ("features", 4, F32), ("rowtab", 4, F32), ("coltab", 4, F32))
def _(v):
    g = geom(P_=1, rowtab=v["rowtab"].value, coltab=v["coltab"].value)
    return L().lbdrn_features(byref(g), v["msb"], v["idx"], 50, v["features"], None)


@entry("lbdrn_forward", ("params", 4, F32), ("x", 4, F32), ("y", 4, F32), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_forward(byref(NET), v["params"], v["x"], 7, v["y"], v["workspace"], BIG, None)


@entry("lbdrn_forward_tape", ("params", 4, F32), ("x", 4, F32), ("y", 4, F32), ("tape", 256, F32))
def _(v):
    return L().lbdrn_forward_tape(byref(NET), v["params"], v["x"], 7, v["y"], v["tape"], BIG, None)


@entry("lbdrn_backward", ("params", 4, F32), ("x", 4, F32), ("tape", 256, F32), ("y", 4, F32), ("dy", 4, F32), ("grads", 4, F32),
       ("dx", 4, F32), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_backward(byref(NET), v["params"], v["x"], 7, v["tape"], BIG, v["y"], v["dy"], v["grads"], v["dx"],
                              v["workspace"], BIG, None)


@entry("lbdrn_decode_fused", ("msb", 2, U16), ("params", 4, F32), ("out", 2, U16), ("y_out", 4, F32), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_decode_fused(byref(G), byref(NET), v["msb"], v["params"], v["out"], v["y_out"], v["workspace"], BIG, 0, None)


@entry("lbdrn_eval_sse", ("img", 2, U16), ("msb", 2, U16), ("params", 4, F32), ("sse", 8, F64), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_eval_sse(byref(G), byref(NET), v["img"], v["msb"], v["params"], v["sse"], v["workspace"], BIG, 0, None)


@entry("lbdrn_train_prepare", ("img", 2, U16), ("msb", 2, U16), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_train_prepare(byref(G), byref(NET), v["img"], v["msb"], 32, v["workspace"], BIG, 0, None)


TRAIN_PTRS = (("img", 2, U16), ("msb", 2, U16), ("perm", 8, I64), ("params", 16, F32), ("exp_avg", 4, F32), ("exp_avg_sq", 4, F32),
              ("losses", 4, F32), ("workspace", 256, F32))


@entry("lbdrn_train_epoch", *TRAIN_PTRS)
def _(v):
    return L().lbdrn_train_epoch(byref(G), byref(NET), v["img"], v["msb"], v["perm"], 100, 32, v["params"], v["exp_avg"],
                                 v["exp_avg_sq"], 0, 1e-3, v["losses"], v["workspace"], BIG, 0, None)


@entry("lbdrn_train_epoch_group", *TRAIN_PTRS)
def _(v):
    """two fits; the SECOND fit's pointer is the one that moves (the first fit's lie 2 MiB below, aligned)"""
    arr = lambda name: (ctypes.c_void_p * 2)(v[name].value - (2 << 20) - (v[name].value % 256), v[name].value)
    garr = (ctypes.POINTER(_lib.Geom) * 2)(ctypes.pointer(G), ctypes.pointer(G))
    return L().lbdrn_train_epoch_group(2, ctypes.cast(garr, ctypes.c_void_p), byref(NET), arr("img"), arr("msb"), arr("perm"), 100, 32,
                                       arr("params"), arr("exp_avg"), arr("exp_avg_sq"), 0, 1e-3, arr("losses"), arr("workspace"),
                                       BIG, 0, None)


@entry("lbdrn_train_step", ("x", 4, F32), ("t", 4, F32), ("params", 4, F32), ("exp_avg", 4, F32), ("exp_avg_sq", 4, F32),
       ("loss", 4, F32), ("grads", 4, F32), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_train_step(byref(NET), v["x"], v["t"], 7, v["params"], v["exp_avg"], v["exp_avg_sq"], 1, 1e-3, 1, v["loss"],
                                v["grads"], v["workspace"], BIG, None)


@entry("lbdrn_randperm", ("perm", 8, I64), ("workspace", 256, F32))
def _(v):
    seeds = (ctypes.c_uint64 * 1)(3)
    return L().lbdrn_randperm(seeds, 1, 1000, v["perm"], v["workspace"], BIG, None)


@entry("lbdrn_plane_encode", ("planes", 2, U16), ("body", 4, 1), ("body_bytes", 8, 8), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_plane_encode(v["planes"], 2, 9, 12, v["body"], BIG, v["body_bytes"], v["workspace"], BIG, None)


@entry("lbdrn_plane_decode", ("body", 4, 1), ("planes", 2, U16), ("status", 4, I32), ("workspace", 256, F32))
def _(v):
    return L().lbdrn_plane_decode(v["body"], 64, 2, 9, 12, v["planes"], v["status"], v["workspace"], BIG, None)


@entry("lbdrn_jp2k_encode", ("planes", 2, U16), ("workspace", 256, F32))
def _(v):
    out, n = (ctypes.c_uint8 * 64)(), ctypes.c_size_t(0)
    return L().lbdrn_jp2k_encode(v["planes"], 2, 9, 12, 16, out, 64, byref(n), v["workspace"], BIG, None)


def _values(pointers, moved=None):
    return {p.name: p.value(p.misplaced() if p is moved else 0) for p in pointers}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_call_at_the_declared_alignments_gets_past_the_argument_checks(name):
    """... and only then asks for the device: the refusals below are about the one pointer that moved"""
    if not no_device():
        pytest.skip("a device is present: a call that passes the checks would launch on addresses that are not memory")
    pointers, call = CALLS[name]
    assert call(_values(pointers)) == E_DEVICE, (name, last_error())
    # the least aligned placement the header allows, every pointer at once: still past the checks
    least = {p.name: p.value(p.align % 256) for p in pointers}
    assert call(least) == E_DEVICE, (name, last_error())


@pytest.mark.parametrize("name,arg", [pytest.param(n, p, id=f"{n}-{p.name}") for n in sorted(CALLS) for p in CALLS[n][0]])
def test_a_pointer_below_its_declared_alignment_is_refused_before_the_device_is_looked_for(name, arg):
    pointers, call = CALLS[name]
    rc = call(_values(pointers, moved=arg))
    assert rc == E_ARG, (name, arg.name, rc, last_error())
    # the message is about this argument alone: it opens with its name (the geometry's tables as g->rowtab / g->coltab, a fit's
    # pointers as "<argument> of fit B": the second fit's is the one that moved) and states its alignment, the only number in it
    msg = last_error()
    subject = {"rowtab": "g->rowtab", "coltab": "g->coltab"}.get(arg.name, arg.name)
    if name == "lbdrn_train_epoch_group":
        subject += " of fit B"
    assert msg.startswith(f"{subject} must be {arg.align}-byte aligned"), (name, arg.name, msg)
    assert re.findall(r"\d+", msg) == [str(arg.align)], msg


def test_every_pointer_argument_of_the_header_has_a_declared_alignment_here():
    """every entry point the hygiene tests count as taking device pointers is in CALLS, lbdrn_jp2k_encode included"""
    device_entries = {"lbdrn_split_bits", "lbdrn_labels", "lbdrn_features", "lbdrn_forward", "lbdrn_forward_tape", "lbdrn_backward",
                      "lbdrn_decode_fused", "lbdrn_eval_sse", "lbdrn_train_prepare", "lbdrn_train_epoch", "lbdrn_train_epoch_group",
                      "lbdrn_randperm", "lbdrn_plane_encode", "lbdrn_plane_decode", "lbdrn_jp2k_encode", "lbdrn_train_step"}
    assert set(CALLS) == device_entries
    for name, (pointers, _) in CALLS.items():
        nvp = sum(1 for a in _lib.SIGNATURES[name][1] if a is ctypes.c_void_p)
        # every void* of the binding but the stream (and, for the group call, the array of geometries; for lbdrn_jp2k_encode,
        # the host output) is a pointer with a declared alignment; lbdrn_features' tables travel inside the geometry
        extra = {"lbdrn_train_epoch_group": 2, "lbdrn_jp2k_encode": 2, "lbdrn_features": -1}.get(name, 1)
        assert len(pointers) == nvp - extra, (name, len(pointers), nvp)


def test_the_weight_payload_calls_ask_four_bytes_of_their_host_values():
    vals = (ctypes.c_float * 9)(*range(9))
    out, n = (ctypes.c_uint8 * 4096)(), ctypes.c_size_t(0)
    assert L().lbdrn_weights_encode(ctypes.c_void_p(ctypes.addressof(vals) + 2), 8, 16, out, 4096, byref(n)) == E_ARG
    assert "values" in last_error() and "4-byte" in last_error()
    assert L().lbdrn_weights_decode(out, 64, ctypes.c_void_p(ctypes.addressof(vals) + 2), 8) == E_ARG
    assert "values" in last_error()


# ---------------------------------------------------------------- the satellite libraries that carve a caller's workspace
#
# lbdrn_resid.h, lbdrn_tiff.h, lbdrn_jp2k_dec.h state: the workspace 256 (its regions are 32- and 64-bit words laid out from the
# base), 16-bit planes 2, status 4, body_bytes 8; bodies, files and 8-bit planes any address.  Same form as above: the call at
# the declared alignments passes the argument checks, the call with ONE pointer moved is LBDRN_E_ARG and names it.

def _sat(k, off=0):
    return ctypes.c_void_p(BASE + 4096 * k + off)


def _resid_encode(v):
    from lbdrn_hip import resid
    return resid, resid.lib().lbdrn_resid_encode(v["orig"], v["recon"], 2, 9, 12, 1, v["body"], BIG, v["body_bytes"], v["workspace"], BIG, None)


def _resid_decode(v):
    from lbdrn_hip import resid
    return resid, resid.lib().lbdrn_resid_decode(v["body"], 4096, 2, 9, 12, 0, 0, 12, 9, v["recon_inout"], v["status"], v["workspace"],
                                                 BIG, None)


def _tiff_decode(v, bits=16):
    from lbdrn_hip import tiff
    lay = tiff.Layout(2, 9, 12, bits, 0, 2, 12, 9, 0, tiff.COMP_DEFLATE, 1)          # two strips of one band each
    nseg = tiff.lib().lbdrn_tiff_segment_count(byref(lay))
    assert nseg == 2
    offsets, counts = np.zeros(nseg, np.uint64), np.full(nseg, 8, np.uint64)          # (host arrays: read before anything else)
    return tiff, tiff.lib().lbdrn_tiff_decode(byref(lay), v["file"], 4096, offsets.ctypes.data, counts.ctypes.data, nseg, v["planes"],
                                              v["status"], v["workspace"], BIG, None)


def _jp2kd_decode(v):
    from lbdrn_hip import jp2k_dec
    buf = b"not a codestream"          # (the pointer checks stand in front of the parser)
    return jp2k_dec, jp2k_dec.lib().lbdrn_jp2kd_decode(buf, len(buf), v["planes"], 2, 9, 12, v["workspace"], BIG, None)


# call -> (its pointer arguments: name, declared alignment (1: none), the offset that leaves it), what passing the checks answers
# here: the device error, or, for the JPEG 2000 decoder, the parser's refusal of a buffer that is no codestream
SATELLITES = {
    "lbdrn_resid_encode": (_resid_encode, [("orig", 2, 1), ("recon", 2, 1), ("body", 1, 1), ("body_bytes", 8, 4), ("workspace", 256, 4)], E_DEVICE),
    "lbdrn_resid_decode": (_resid_decode, [("body", 1, 1), ("recon_inout", 2, 1), ("status", 4, 2), ("workspace", 256, 4)], E_DEVICE),
    "lbdrn_tiff_decode": (_tiff_decode, [("file", 1, 1), ("planes", 2, 1), ("status", 4, 2), ("workspace", 256, 4)], E_DEVICE),
    "lbdrn_jp2kd_decode": (_jp2kd_decode, [("planes", 2, 1), ("workspace", 256, 4)], E_ARG),
}


def _sat_values(args, moved=None):
    return {name: _sat(k + 1, off if name == moved else 0) for k, (name, align, off) in enumerate(args)}


@pytest.mark.parametrize("entry,arg", [pytest.param(e, a, id=f"{e}-{a[0]}") for e in SATELLITES for a in SATELLITES[e][1]])
def test_satellite_libraries_refuse_a_pointer_below_its_declared_alignment(entry, arg):
    call, args, passed = SATELLITES[entry]
    name, align, off = arg
    if align == 1:     # no alignment declared: an odd address passes the checks like an even one
        if not no_device():
            pytest.skip("a device is present: a call that passes the checks would launch on addresses that are not memory")
        mod, rc = call(_sat_values(args, moved=name))
        assert rc == passed, (entry, name, rc, mod._NATIVE.last_error())
        return
    mod, rc = call(_sat_values(args, moved=name))
    msg = mod._NATIVE.last_error()
    assert rc == E_ARG and msg == f"{entry}: {name} is not {align}-byte aligned", (entry, name, rc, msg)


@pytest.mark.parametrize("entry", sorted(SATELLITES))
def test_satellite_calls_at_the_declared_alignments_get_past_the_pointer_checks(entry):
    if not no_device():
        pytest.skip("a device is present: a call that passes the checks would launch on addresses that are not memory")
    call, args, passed = SATELLITES[entry]
    mod, rc = call(_sat_values(args))
    assert rc == passed and "aligned" not in mod._NATIVE.last_error(), (entry, rc, mod._NATIVE.last_error())


def test_tiff_planes_of_8_bit_samples_need_no_alignment():
    if not no_device():
        pytest.skip("a device is present: a call that passes the checks would launch on addresses that are not memory")
    args = SATELLITES["lbdrn_tiff_decode"][1]
    mod, rc = _tiff_decode(_sat_values(args, moved="planes"), bits=8)
    assert rc == E_DEVICE, mod._NATIVE.last_error()


# ---------------------------------------------------------------- NULL msb with LBDRN_EVAL_FAST

FAST, X16, BG = _lib.EVAL_FAST, _lib.EVAL_X16, _lib.EVAL_BACKGROUND


def eval_null_msb(g, net, word):
    img, params, sse, ws = (ctypes.c_void_p(BASE + 4096 * k) for k in range(1, 5))
    return L().lbdrn_eval_sse(byref(g), byref(net), img, None, params, sse, ws, BIG, word, None)


def shape(C, H, W, bc, D=2, nl=2, act=0):
    g = geom(C=C, H=H, W=W, D=D)
    return g, net_of(g, bc=bc, nl=nl, act=act)


@pytest.mark.parametrize("word,why", [(_lib.PATH_AUTO, "only LBDRN_EVAL_FAST"), (_lib.PATH_MFMA, "only LBDRN_EVAL_FAST"),
                                      (_lib.PATH_MFMA | BG, "only LBDRN_EVAL_FAST"), (_lib.PATH_GENERIC, "only LBDRN_EVAL_FAST"),
                                      (_lib.PATH_GENERIC | FAST, "generic path"), (_lib.PATH_GENERIC | FAST | X16, "generic path")])
def test_null_msb_is_refused_without_the_flag_and_on_the_generic_path(word, why):
    g, net = shape(4, 130, 70, 64)
    assert eval_null_msb(g, net, word) == E_ARG
    assert "msb must not be null" in last_error() and why in last_error(), last_error()


def test_null_msb_is_refused_where_path_auto_takes_the_generic_kernels():
    """bc = 48 has no fused apply kernel: LBDRN_PATH_AUTO | LBDRN_EVAL_FAST runs the generic pass, which reads msb"""
    g, net = shape(3, 17, 37, 48)
    assert eval_null_msb(g, net, _lib.PATH_AUTO | FAST) == E_ARG and "generic path" in last_error()


@pytest.mark.parametrize("C,bc", [(10, 64), (10, 32), (9, 64), (16, 64), (1, 128), (4, 128)])
@pytest.mark.parametrize("flags", (FAST, FAST | X16, FAST | BG), ids=("fast", "fast_x16", "fast_background"))
def test_null_msb_is_refused_for_a_fast_request_that_a_canonical_instance_serves(C, bc, flags):
    """more than 8 bands on k_apply_mfma (apply_mfma.hip: `mode_fast(mode) && net.C > 8`), and bc = 128, which has no fast
    instance (APPLY_INSTANCES): serving_mode answers MODE_EVAL, and that instance reads msb"""
    g, net = shape(C, 20, 70, bc)
    for path in (_lib.PATH_AUTO, _lib.PATH_MFMA):
        assert eval_null_msb(g, net, path | flags) == E_ARG, (C, bc, path)
        assert "canonical instance" in last_error(), last_error()


@pytest.mark.parametrize("C,H,W,bc", [(3, 17, 200, 32), (4, 130, 70, 64), (8, 48, 64, 256), (1, 9, 9, 64), (8, 20, 70, 32), (2, 2, 70001, 64), (8, 20, 70, 128)])
@pytest.mark.parametrize("flags", (FAST, FAST | X16, FAST | BG), ids=("fast", "fast_x16", "fast_background"))
def test_null_msb_passes_the_argument_check_where_a_fast_instance_serves(C, H, W, bc, flags):
    """the fused families of tests/test_gpu_workspace_hygiene.py's APPLY_SHAPES with a fast instance: the call gets past the
    argument check and asks for the device.  (8 bands at bc = 128: the weights do not fit in LDS beside the window, the
    streaming kernel serves the shape, and its fast instance takes img >> K -- the same width refused above at 1 and 4 bands.)"""
    if not no_device():
        pytest.skip("a device is present: the call would launch on addresses that are not memory")
    g, net = shape(C, H, W, bc)
    for path in (_lib.PATH_AUTO, _lib.PATH_MFMA):
        assert eval_null_msb(g, net, path | flags) == E_DEVICE, (path, last_error())


def test_img_params_and_sse_stay_mandatory_with_the_flag():
    g, net = shape(4, 130, 70, 64)
    a = [ctypes.c_void_p(BASE + 4096 * k) for k in range(1, 5)]
    for k in range(3):
        args = list(a[:3])
        args[k] = None
        img, params, sse = args
        assert L().lbdrn_eval_sse(byref(g), byref(net), img, None, params, sse, a[3], BIG, _lib.PATH_MFMA | FAST, None) == E_ARG


# ---------------------------------------------------------------- minibatch sizes up to INT32_MAX

INT_MAX = 2 ** 31 - 1


def train_ws(g, net, bs):
    return int(L().lbdrn_train_workspace(byref(g), byref(net), bs))


@pytest.mark.parametrize("C,H,W,bc,D,nl", [(8, 9, 12, 64, 2, 2), (8, 256, 256, 64, 2, 2), (3, 25, 33, 64, 1, 3), (8, 12, 15, 64, 3, 2),
                                           (4, 30, 41, 128, 2, 1), (8, 40, 52, 256, 2, 2), (3, 9, 12, 48, 2, 2)],
                         ids=("headline_9x12", "headline_256x256", "nl3", "wide_window", "bc128", "bc256", "generic_bc48"))
def test_train_workspace_is_exact_up_to_int32_max_rows(C, H, W, bc, D, nl):
    """The sizing is host integer arithmetic, restated in Python integers (which do not wrap) by tests/wide_plan_reference.py:
    carve_train of csrc/generic.hip and wide_ws_layout of csrc/train_wide.inc.  EXACT wherever those two decide the size: at
    every minibatch size for bc = 128 / 256 (the larger of the two) and for a width without a fused step (the generic one), and
    for the fused bc = 64 step at the sizes whose slabs pass 2 GiB -- there LBDRN_PATH_MFMA is refused BY SIZE and the generic
    layout is all there is, so the equality also pins that the refusal came from the true count and not from a wrapped one
    (`bs + 31` and `bs + 255` used to leave int: the sizes near 2^31 - 1 came out as those of a few rows).  Below 2 GiB the
    bc = 64 layout is train_ws_layout's, which has no restatement: it is held between the generic size and 64 KiB a row more
    (a loose bracket, a smoke check of the order of magnitude), and the test below pins its increments."""
    import train_plan_reference as R
    import wide_plan_reference as WR
    g, net = shape(C, H, W, bc, D=D, nl=nl)
    s = R.Shape(0, 0, 1, 1, C, D, nl, "sine")
    assert s.F == net.F
    near = (INT_MAX - 300, INT_MAX - 255, INT_MAX - 31, INT_MAX)
    for bs in (1, H * W, H * W + 1, 10 ** 6) + near:
        got, generic = train_ws(g, net, bs), WR.generic_workspace_bytes(s, bc, bs)
        if bc in WR.BCS:
            assert got == WR.workspace_bytes(s, bc, H, W, bs), (bs, got)
        elif bc != 64 or bs in near:
            assert got == generic, (bs, got, generic)
        else:
            assert generic <= got <= generic + H * W * 4096 + bs * 65536 + (64 << 20), (bs, got, generic)


def test_fused_train_workspace_grows_in_equal_steps():
    """the fused bc = 64 step, where its layout decides the size (below the 2 GiB of slabs): 1024 more rows are 32 more
    workgroups -- 32 slabs in each rotating set, 256 bytes of loss partials, 1024 staged rows twice -- the same increment
    wherever it is taken (csrc/train_mfma.hip train_ws_layout), and more than the generic step's for the same rows"""
    import train_plan_reference as R
    import wide_plan_reference as WR
    g, net = shape(8, 256, 256, 64)
    s = R.Shape(0, 0, 1, 1, 8, 2, 2, "sine")
    step = lambda bs: train_ws(g, net, bs + 1024) - train_ws(g, net, bs)
    assert step(1024 * 8) == step(1024 * 64) == step(1024 * 512)
    assert step(1024 * 8) > WR.generic_workspace_bytes(s, 64, 2048) - WR.generic_workspace_bytes(s, 64, 1024)
