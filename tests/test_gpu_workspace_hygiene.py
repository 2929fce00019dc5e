"""Poisoned-workspace and guard-band tests for every device entry point of include/lbdrn_hip.h.

The header calls every workspace "device scratch" and says the library keeps no state: what a workspace, a tape or an
output buffer holds on entry must not matter, and nothing beyond the declared size may be touched.  The rest of the suite
hands the kernels `torch.empty` buffers -- zeros from a fresh block, or finite floats a previous test left -- which hide a
kernel that reads a pad column, a ragged tail row, an absent workgroup's partial or an alignment gap before anything wrote
it (0 x finite = 0, but 0 x NaN = NaN).  Here every entry point runs once per fill (tests/guarded.py: 0x00, 0xFF, 0xA5)
of its scratch AND its output buffers, on the same inputs, through ctypes so that the test owns every byte, and

  (a) every output is bit-identical across the three fills,
  (b) every guard (64 KiB in front of and behind every buffer, in the same allocation) is intact,
  (c) the 0x00-fill result passes the check the suite already applies to that entry point, at that check's tolerance
      (three runs that agree on a wrong answer do not pass),
  (d) const inputs hold the same bits after the call,
  (e) workspace_bytes is exactly what the sizing function returned.

The test ids read <entry point>-<kernel family / shape>-<fill>.  Within a case the 0x00 fill runs first.

lbdrn_eval_sse and *sse: the header says the call OVERWRITES *sse on every path (csrc/generic.hip: k_sum_partials with
accumulate = 0 on the first chunk; csrc/apply_mfma.hip: k_sum_partials_mfma, `*dst = s`), so *sse is an output like any
other here: it is poisoned with the fill before the call."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import oracle as O
from guarded import FILLS, Arena, fill_id
from lbdrn_hip import _lib, ops
from lbdrn_hip.features import FeatCfg
from test_gpu_autograd import _nrel, _restated
from test_gpu_fuzz import _params
from test_gpu_plane_codec import _oracle_body
from lbdrn_hip.synth import synthetic_tile

pytestmark = pytest.mark.gpu
GEN, MFMA = _lib.PATH_GENERIC, _lib.PATH_MFMA
byref = ctypes.byref


def L():
    return _lib.lib()


def call(dev, fn, *args):
    """one C entry point on the current stream of `dev`, synchronised; returns its status"""
    with torch.cuda.device(dev):
        rc = fn(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    return rc


def ok(rc):
    assert rc == 0, (rc, (L().lbdrn_last_error() or b"").decode())


def align_up(n, a=256):
    return (n + a - 1) // a * a


def ocfg_of(cfg):
    return O.FeatCfg(cfg.use_coordinates, cfg.embedding, 1.4, 12, cfg.use_colors, cfg.relative)


def make_cfg(flags, act="sine"):
    return FeatCfg(bool(flags[0]), bool(flags[1]), 1.4, 12, bool(flags[2]), bool(flags[3]), act)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Case:
    """run(dev, fill) -> {name: numpy array}: one call on guarded buffers, (b) (d) (e) asserted inside;
    check(dev, outs): (c) on the 0x00-fill result"""

    def __init__(self, entry, family, run, check):
        self.id, self.run, self.check = f"{entry}-{family}", run, check


CASES = []
_BASE = {}


def case(entry, family):
    def deco(make):
        run, check = make()
        CASES.append(Case(entry, family, run, check))
        return make
    return deco


# =============================================================== a1 - a3: split_bits, labels, features (outputs only)

K_IMG = 5
IMG_SHAPES = [(1, 7, 13, 0), (5, 9, 31, 3), (1, 9, 31, 3), (5, 7, 13, 0)]      # C, H, W (odd), D
CFG_FLAGS = [("relative", (0, 0, 1, 1)), ("absolute", (0, 0, 1, 0)), ("coords", (1, 0, 1, 1)), ("embedding", (1, 1, 1, 0)),
             ("embedding_no_colours", (1, 1, 0, 0))]


def small_image(seed, C, H, W):
    img = np.random.default_rng(seed).integers(0, 10001, (C, H, W)).astype(np.uint16)
    img[0, 0, 0] |= np.uint16(1 << K_IMG)
    return img


def add_split_bits(C, H, W, with_msb):
    @case("lbdrn_split_bits", f"C{C}_{H}x{W}_" + ("msb" if with_msb else "max_only"))
    def _():
        img = small_image(C, C, H, W)

        def run(dev, fill):
            A = Arena(dev)
            src = A.const(img, "img")
            msb = A.buf(img.nbytes, fill, name="msb") if with_msb else None
            mx = A.buf(4, 0x00, name="msb_max")          # in/out: the caller zeroes it (lbdrn_hip.h), whatever the fill
            ok(call(dev, L().lbdrn_split_bits, src.ptr, C, H, W, K_IMG, msb.ptr if msb else None, mx.ptr))
            A.check()
            return {"msb": msb.numpy(np.uint16) if msb else np.zeros(0, np.uint16), "max": mx.numpy(np.int32)}

        def check(dev, outs):
            msb_o, _, mx = O.split_bits(img, K_IMG)
            assert int(outs["max"][0]) == mx
            if with_msb:
                assert np.array_equal(outs["msb"], msb_o.reshape(-1))
        return run, check


def add_labels(C, H, W, use_idx):
    @case("lbdrn_labels", f"C{C}_{H}x{W}_" + ("idx" if use_idx else "raster"))
    def _():
        img = small_image(10 + C, C, H, W)
        idx = np.random.default_rng(C).integers(0, H * W, 50).astype(np.int64) if use_idx else None
        n = 50 if use_idx else H * W

        def run(dev, fill):
            A = Arena(dev)
            src = A.const(img, "img")
            ix = A.const(idx, "idx") if use_idx else None
            out = A.buf(n * C * 4, fill, name="labels")
            ok(call(dev, L().lbdrn_labels, src.ptr, C, H, W, K_IMG, ix.ptr if ix else None, n, out.ptr))
            A.check()
            return {"labels": out.numpy(np.float32)}

        def check(dev, outs):
            _, lab, _ = O.split_bits(img, K_IMG)
            want = lab[idx] if use_idx else lab
            assert bits_equal(outs["labels"], np.ascontiguousarray(want, np.float32).reshape(-1))
        return run, check


def add_features(shape, name, flags, use_idx):
    C, H, W, D = shape

    @case("lbdrn_features", f"C{C}_D{D}_{H}x{W}_{name}_" + ("idx" if use_idx else "raster"))
    def _():
        cfg = make_cfg(flags)
        img = small_image(20 + C + D, C, H, W)
        msb_np, _, mx = O.split_bits(img, K_IMG)
        idx = np.random.default_rng(D).integers(0, H * W, 77).astype(np.int64) if use_idx else None
        n = 77 if use_idx else H * W
        F = cfg.feature_dim(C, D)

        def run(dev, fill):
            A = Arena(dev)
            geom = ops.FeatureGeometry(C, H, W, K_IMG, D, mx, cfg, dev)
            msb = A.const(msb_np, "msb")
            ix = A.const(idx, "idx") if use_idx else None
            out = A.buf(n * F * 4, fill, name="features")
            ok(call(dev, L().lbdrn_features, byref(geom.c), msb.ptr, ix.ptr if ix else None, n, out.ptr))
            A.check()
            return {"features": out.numpy(np.float32)}

        def check(dev, outs):
            want = O.features(msb_np, D, ocfg_of(cfg), mx)
            want = want[idx] if use_idx else want
            assert bits_equal(outs["features"], np.ascontiguousarray(want, np.float32).reshape(-1))
        return run, check


add_split_bits(1, 7, 13, True)
add_split_bits(5, 9, 31, True)
add_split_bits(5, 9, 31, False)
for _C, _H, _W in ((1, 7, 13), (5, 9, 31)):
    for _u in (True, False):
        add_labels(_C, _H, _W, _u)
for _i, (_name, _flags) in enumerate(CFG_FLAGS):
    for _j, _u in enumerate((True, False)):
        add_features(IMG_SHAPES[(2 * _i + _j) % 4], _name, _flags, _u)


# =============================================================== a5, autograd, the teacher-forced step (any width)

# (bc, B, activation): the fuzz's widths that leave ragged GEMM tiles and batches that need a split-K reduction
NET_SHAPES = [(7, 4097, "sine", 37, 5, 2), (65, 65, "relu", 200, 8, 1), (200, 1, "relu", 37, 5, 3), (300, 4097, "sine", 61, 3, 2),
              (65, 1, "sine", 9, 1, 2), (200, 65, "sine", 200, 8, 2), (300, 65, "relu", 37, 5, 1), (7, 65, "relu", 61, 3, 3)]


def net_inputs(bc, B, act, F, C, nl):
    rng = np.random.default_rng(bc * 10007 + B)
    pn = _params(rng, F, bc, C, nl, 30.0 if act == "relu" else 1.5)
    x = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    t = rng.uniform(0, 1, (B, C)).astype(np.float32)
    net = ops.make_net(F, bc, C, nl, ops.ACT_RELU if act == "relu" else ops.ACT_SINE)
    return pn, x, t, net


def net_family(bc, B, act, F, C, nl):
    return f"bc{bc}_B{B}_{act}_F{F}_C{C}_nl{nl}"


def add_forward(shape):
    bc, B, act, F, C, nl = shape

    @case("lbdrn_forward", net_family(*shape))
    def _():
        pn, x, t, net = net_inputs(*shape)

        def run(dev, fill):
            A = Arena(dev)
            p, xd = A.const(pn, "params"), A.const(x, "x")
            y = A.buf(B * C * 4, fill, name="y")
            nws = L().lbdrn_forward_workspace(byref(net), B)
            ws = A.buf(nws, fill, name="workspace")
            ok(call(dev, L().lbdrn_forward, byref(net), p.ptr, xd.ptr, B, y.ptr, ws.ptr, nws))
            A.check()
            return {"y": y.numpy(np.float32)}

        def check(dev, outs):
            with O.hidden_activation(act):
                yo = O.forward(pn, F, bc, C, nl, x)
            assert bits_equal(outs["y"], yo.reshape(-1))
        return run, check


def run_forward_tape(dev, A, fill, net, pn, x, B):
    """lbdrn_forward_tape into a poisoned tape; returns (params, x, y, tape, tape_bytes)"""
    C = net.C
    p, xd = A.const(pn, "params"), A.const(x, "x")
    y = A.buf(B * C * 4, fill, name="y")
    nt = L().lbdrn_tape_bytes(byref(net), B)
    tape = A.buf(nt, fill, name="tape")
    ok(call(dev, L().lbdrn_forward_tape, byref(net), p.ptr, xd.ptr, B, y.ptr, tape.ptr, nt))
    return p, xd, y, tape, nt


def add_forward_tape(shape):
    bc, B, act, F, C, nl = shape

    @case("lbdrn_forward_tape", net_family(*shape))
    def _():
        pn, x, t, net = net_inputs(*shape)

        def run(dev, fill):
            A = Arena(dev)
            p, xd, y, tape, nt = run_forward_tape(dev, A, fill, net, pn, x, B)
            A.check()
            half, used = align_up(nl * B * bc * 4), nl * B * bc
            assert nt == 2 * half
            raw = tape.numpy(np.float32)
            # the regions the header names (hidden outputs, their derivatives); the alignment gaps behind them keep the fill
            return {"y": y.numpy(np.float32), "hidden": raw[:used], "derivative": raw[half // 4:half // 4 + used]}

        def check(dev, outs):
            with O.hidden_activation(act):
                yo = O.forward(pn, F, bc, C, nl, x)
            assert bits_equal(outs["y"], yo.reshape(-1))
        return run, check


def add_backward(shape, want_dx):
    bc, B, act, F, C, nl = shape

    @case("lbdrn_backward", net_family(*shape) + ("_dx" if want_dx else "_no_dx"))
    def _():
        pn, x, t, net = net_inputs(*shape)
        dy_of = lambda yh: (np.float32(2) * (yh.reshape(B, C) - t)) * (np.float32(1) / (np.float32(B) * np.float32(C)))

        def run(dev, fill):
            A = Arena(dev)
            p, xd, y, tape, nt = run_forward_tape(dev, A, fill, net, pn, x, B)     # the tape's gaps carry the poison
            tape_before, y_before = tape.numpy(np.uint8), y.numpy(np.uint8)
            dy = A.const(dy_of(y.numpy(np.float32)), "dy")
            NP = ops.param_count(net)
            grads = A.buf(NP * 4, fill, name="grads")
            dx = A.buf(B * F * 4, fill, name="dx") if want_dx else None
            nws = L().lbdrn_backward_workspace(byref(net), B)
            ws = A.buf(nws, fill, name="workspace")
            ok(call(dev, L().lbdrn_backward, byref(net), p.ptr, xd.ptr, B, tape.ptr, nt, y.ptr, dy.ptr, grads.ptr,
                    dx.ptr if dx else None, ws.ptr, nws))
            A.check()
            assert np.array_equal(tape.numpy(np.uint8), tape_before), "lbdrn_backward wrote to its const tape"
            assert np.array_equal(y.numpy(np.uint8), y_before), "lbdrn_backward wrote to its const y"
            return {"grads": grads.numpy(np.float32), "dx": dx.numpy(np.float32) if dx else np.zeros(0, np.float32),
                    "y": y.numpy(np.float32)}

        def check(dev, outs):
            # the header's statement, as tests/test_gpu_autograd.py holds it: with dy the MSE gradient, lbdrn_train_step's grads
            p, xd, td = (torch.from_numpy(a).to(dev) for a in (pn, x, t))
            _, g_ref = ops.train_step(net, xd, td, p, torch.zeros_like(p), torch.zeros_like(p), 1, 1e-3, apply_adam=False)
            assert bits_equal(outs["grads"], g_ref.cpu().numpy())
            if want_dx:   # dL/dx against the float64 restatement, test_arbitrary_upstream_gradient_and_input_gradient_vs_float64's bound
                p64 = torch.from_numpy(pn).double()
                x64 = torch.from_numpy(x).double().requires_grad_()
                y64 = _restated(p64, x64, F, bc, C, nl, act == "relu")
                (y64 * torch.from_numpy(dy_of(outs["y"])).double()).sum().backward()
                want = x64.grad.numpy()
                if np.linalg.norm(want) > 0:
                    assert _nrel(outs["dx"].reshape(B, F), want) <= 2e-5, _nrel(outs["dx"].reshape(B, F), want)
                else:
                    assert not outs["dx"].any()
        return run, check


def train_step_workspace(net, B):
    g = _lib.Geom(net.C, 1, 1, 1, 0, 1, 1, 1, 0, 0, None, None)      # as ops.train_step sizes it
    return L().lbdrn_train_workspace(byref(g), byref(net), B)


def add_train_step(shape):
    bc, B, act, F, C, nl = shape

    @case("lbdrn_train_step", net_family(*shape))
    def _():
        pn, x, t, net = net_inputs(*shape)

        def run(dev, fill):
            A = Arena(dev)
            xd, td = A.const(x, "x"), A.const(t, "t")
            NP = pn.size
            p = A.buf(NP * 4, 0x00, name="params").write(pn)                 # in/out: the optimiser state is the caller's
            m, v = A.buf(NP * 4, 0x00, name="exp_avg"), A.buf(NP * 4, 0x00, name="exp_avg_sq")
            loss, grads = A.buf(4, fill, name="loss"), A.buf(NP * 4, fill, name="grads")
            nws = train_step_workspace(net, B)
            ws = A.buf(nws, fill, name="workspace")
            ok(call(dev, L().lbdrn_train_step, byref(net), xd.ptr, td.ptr, B, p.ptr, m.ptr, v.ptr, 1, 1e-3, 1, loss.ptr,
                    grads.ptr, ws.ptr, nws))
            A.check()
            return {k: b.numpy(np.float32) for k, b in (("loss", loss), ("grads", grads), ("params", p), ("exp_avg", m), ("exp_avg_sq", v))}

        def check(dev, outs):   # test_forward_and_step_fuzz_any_width_equal_oracle's bounds
            po, mo, vo = pn.copy(), np.zeros_like(pn), np.zeros_like(pn)
            with O.hidden_activation(act):
                lo, go = O.train_step(po, mo, vo, F, bc, C, nl, x, t, 1e-3, 1)
            assert abs(float(outs["loss"][0]) - lo) <= 1e-5 * abs(lo)
            assert np.abs(outs["grads"] - go).max() <= 2e-5 * np.abs(go).max() + 1e-12
            assert np.abs(outs["exp_avg"] - mo).max() <= 2e-5 * np.abs(mo).max() + 1e-12
        return run, check


for _s in NET_SHAPES:
    add_forward(_s)
    add_forward_tape(_s)
    add_backward(_s, False)
    add_backward(_s, True)
    add_train_step(_s)


# =============================================================== a2 + a5 + a11 / a9: decode_fused, eval_sse

# family, path, bc, (C, H, W): tiles ragged in both directions, rasters with fewer tiles than CUs; K = 5, D = 2
APPLY_SHAPES = [("generic_bc32", GEN, 32, (3, 17, 37)), ("k_apply_mfma_bc32", MFMA, 32, (3, 17, 200)),
                ("k_apply_mfma_bc64", MFMA, 64, (4, 130, 70)), ("k_apply_mfma_bc128", MFMA, 128, (1, 9, 9)),
                ("k_apply_wide_bc256", MFMA, 256, (8, 48, 64))]
EVAL_FLAGS = [("canonical", 0), ("background", _lib.EVAL_BACKGROUND), ("fast", _lib.EVAL_FAST),
              ("fast_x16", _lib.EVAL_FAST | _lib.EVAL_X16)]


def apply_inputs(bc, shape):
    C, H, W = shape
    cfg = FeatCfg()
    img = synthetic_tile(7 + C, C, H, W)
    msb, lab, mx = O.split_bits(img, 5)
    F = cfg.feature_dim(C, 2)
    pn = _params(np.random.default_rng(bc + C), F, bc, C, 2, 2.5)
    return cfg, img, msb, lab, mx, F, pn, ops.make_net(F, bc, C, 2)


def add_decode(family, path, bc, shape, want_y):
    C, H, W = shape

    @case("lbdrn_decode_fused", f"{family}_{C}x{H}x{W}_" + ("y_out" if want_y else "y_null"))
    def _():
        cfg, img, msb_np, lab, mx, F, pn, net = apply_inputs(bc, shape)

        def run(dev, fill):
            A = Arena(dev)
            geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, cfg, dev)
            msb, p = A.const(msb_np, "msb"), A.const(pn, "params")
            out = A.buf(C * H * W * 2, fill, name="out")
            y = A.buf(H * W * C * 4, fill, name="y_out") if want_y else None
            nws = L().lbdrn_apply_workspace(byref(geom.c), byref(net))
            ws = A.buf(nws, fill, name="workspace")
            ok(call(dev, L().lbdrn_decode_fused, byref(geom.c), byref(net), msb.ptr, p.ptr, out.ptr, y.ptr if y else None,
                    ws.ptr, nws, path))
            A.check()
            return {"out": out.numpy(np.uint16), "y": y.numpy(np.float32) if y else np.zeros(0, np.float32)}

        def check(dev, outs):   # test_gpu_parity.py: the raster and the sigmoid outputs are the oracle's, bit for bit
            out_o, y_o = O.decode(msb_np, 5, 2, ocfg_of(cfg), pn, bc, 2, mx, want_y=True)
            assert np.array_equal(outs["out"], out_o.reshape(-1))
            if want_y:
                assert bits_equal(outs["y"], np.ascontiguousarray(y_o, np.float32).reshape(-1))
        return run, check


def add_eval(family, path, bc, shape, flag_name, flags):
    C, H, W = shape

    @case("lbdrn_eval_sse", f"{family}_{C}x{H}x{W}_{flag_name}")
    def _():
        cfg, img, msb_np, lab, mx, F, pn, net = apply_inputs(bc, shape)

        def run(dev, fill):
            A = Arena(dev)
            geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, cfg, dev)
            src, msb, p = A.const(img, "img"), A.const(msb_np, "msb"), A.const(pn, "params")
            sse = A.buf(8, fill, name="sse")           # overwritten by the call (module docstring)
            nws = L().lbdrn_apply_workspace(byref(geom.c), byref(net))
            ws = A.buf(nws, fill, name="workspace")
            ok(call(dev, L().lbdrn_eval_sse, byref(geom.c), byref(net), src.ptr, msb.ptr, p.ptr, sse.ptr, ws.ptr, nws, path | flags))
            A.check()
            return {"sse": sse.numpy(np.float64)}

        def check(dev, outs):
            got = float(outs["sse"][0])
            sse_o = O.eval_sse(msb_np, lab, 2, ocfg_of(cfg), pn, bc, 2, mx)
            if flags & _lib.EVAL_FAST:   # lbdrn_hip.h: within 1e-6 relative of the flagless call (itself held to the oracle)
                geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, cfg, dev)
                canon = float(ops.eval_sse(geom, net, ops.to_device_u16(img, dev), ops.to_device_u16(msb_np, dev),
                                           torch.from_numpy(pn).to(dev), path=path).item())
                assert abs(canon - sse_o) <= 1e-11 * max(1.0, abs(sse_o)), (canon, sse_o)
                assert abs(got - canon) <= 1e-6 * canon, (got, canon)
            else:                        # test_gpu_parity.py's bound
                assert abs(got - sse_o) <= 1e-11 * max(1.0, abs(sse_o)), (got, sse_o)
        return run, check


for _fam, _path, _bc, _shape in APPLY_SHAPES:
    for _wy in (True, False):
        add_decode(_fam, _path, _bc, _shape, _wy)
    for _fn, _fl in EVAL_FLAGS:
        add_eval(_fam, _path, _bc, _shape, _fn, _fl)


# =============================================================== a4 + a5 + a7 + a8: prepare + two epochs

# family, path, (C, H, W, K, D, nl, flags), bc, activation, batch size, rows per epoch.  Shapes: CASES of test_gpu_train_paths.py
# and the wide-window shapes of test_gpu_wide_window.py; batch sizes and row counts leave a half-filled last workgroup
# (tails of 17, 33, 49), a ONE-row last minibatch (n = 2 bs + 1) and minibatches shorter than a workgroup (bs = 20).
REL, ABS, EMB = (0, 0, 1, 1), (0, 0, 1, 0), (1, 1, 1, 1)
TRAIN_SHAPES = [
    ("generic_F100", GEN, (4, 30, 41, 5, 2, 2, REL), 64, "sine", 300, 617),
    ("k_train_stream_split_LQ48", MFMA, (8, 40, 52, 5, 2, 2, REL), 64, "sine", 512, 1025),
    ("k_train_stream_split_LQ48_short_minibatch", MFMA, (8, 40, 52, 5, 2, 2, REL), 64, "sine", 20, 41),
    ("k_train_stream_LQ52", MFMA, (8, 40, 52, 5, 2, 2, ABS), 64, "sine", 512, 1073),
    ("k_train_stream_LQ24_nl1", MFMA, (4, 30, 41, 5, 2, 1, REL), 64, "sine", 300, 601),
    ("k_train_stream_split_LQ24", MFMA, (4, 30, 41, 5, 2, 2, REL), 64, "sine", 300, 617),
    ("k_train_stream_LQ32", MFMA, (5, 30, 41, 5, 2, 2, REL), 64, "sine", 300, 633),
    ("k_train_nl3", MFMA, (3, 25, 33, 3, 1, 3, REL), 64, "sine", 256, 513),
    ("k_train_stream_split_LQ64_embedding", MFMA, (8, 24, 36, 5, 2, 2, EMB), 64, "sine", 400, 817),
    ("k_train_stream_split_LQ24_relu", MFMA, (4, 30, 41, 5, 2, 2, REL), 64, "relu", 300, 601),
    ("k_train_split_wide_window_C6", MFMA, (6, 12, 15, 5, 3, 2, REL), 64, "sine", 33, 67),
    ("k_train_split_wide_window_C7", MFMA, (7, 12, 15, 5, 3, 2, REL), 64, "sine", 64, 129),
    ("k_train_split_wide_window_C8", MFMA, (8, 12, 15, 5, 3, 2, REL), 64, "relu", 20, 41),
    ("k_train_half_k_dw_wide_bc128_nl1_3_workgroups", MFMA, (4, 30, 41, 5, 2, 1, REL), 128, "sine", 96, 193),
    ("k_train_half_k_dw_wide_bc256_11_workgroups", MFMA, (8, 40, 52, 5, 2, 2, REL), 256, "sine", 352, 721),
]


def train_inputs(shape, bc, act, n, seed=0):
    C, H, W, K, D, nl, flags = shape
    cfg = make_cfg(flags, act)
    rng = np.random.default_rng(C * 1000 + H + bc + seed)
    img = synthetic_tile(int(rng.integers(100)), C, H, W)
    msb, lab, mx = O.split_bits(img, K)
    F = cfg.feature_dim(C, D)
    p0 = _params(rng, F, bc, C, nl, 10.0 if cfg.act else 1.0)
    perm = rng.permutation(H * W).astype(np.int64)[:n]
    assert len(perm) == n
    return cfg, img, msb, lab, mx, F, p0, perm, ops.make_net(F, bc, C, nl, cfg.act)


class Fit:
    """one fit's guarded buffers: optimiser state, losses, workspace (poisoned BEFORE lbdrn_train_prepare, untouched after)"""

    def __init__(self, A, dev, fill, shape, cfg, img, msb, mx, p0, perm, net, bs, tag="", ws=None):
        C, H, W, K, D, nl, flags = shape
        self.geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
        self.net, self.bs, self.n = net, bs, len(perm)
        self.steps = (self.n + bs - 1) // bs
        self.img, self.msb, self.perm = A.const(img, "img" + tag), A.const(msb, "msb" + tag), A.const(perm, "perm" + tag)
        NP = p0.size
        self.p = A.buf(NP * 4, 0x00, name="params" + tag).write(p0)
        self.m, self.v = A.buf(NP * 4, 0x00, name="exp_avg" + tag), A.buf(NP * 4, 0x00, name="exp_avg_sq" + tag)
        self.losses = A.buf(self.steps * 4, fill, name="losses" + tag)
        self.nws = L().lbdrn_train_workspace(byref(self.geom.c), byref(net), bs)
        assert self.nws > 0
        self.ws = ws if ws is not None else A.buf(self.nws, fill, name="workspace" + tag)
        assert self.ws.nbytes >= self.nws

    def prepare(self, dev, path):
        ok(call(dev, L().lbdrn_train_prepare, byref(self.geom.c), byref(self.net), self.img.ptr, self.msb.ptr, self.bs,
                self.ws.ptr, self.nws, path))

    def epoch(self, dev, e, path):
        ok(call(dev, L().lbdrn_train_epoch, byref(self.geom.c), byref(self.net), self.img.ptr, self.msb.ptr, self.perm.ptr,
                self.n, self.bs, self.p.ptr, self.m.ptr, self.v.ptr, e * self.steps, 1e-3, self.losses.ptr, self.ws.ptr,
                self.nws, path))

    def outs(self, tag=""):
        return {k + tag: b.numpy(np.float32) for k, b in (("params", self.p), ("exp_avg", self.m), ("exp_avg_sq", self.v),
                                                           ("losses", self.losses))}


def epochs_through_ops(dev, shape, cfg, img, msb, mx, p0, perm, net, bs, path, epochs=2):
    """the same fit through lbdrn_hip.ops on buffers of its own -> params, exp_avg, exp_avg_sq, losses"""
    C, H, W, K, D, nl, flags = shape
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    img_d, msb_d = ops.to_device_u16(img, dev), ops.to_device_u16(msb, dev)
    steps = (len(perm) + bs - 1) // bs
    p = torch.from_numpy(p0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img_d, msb_d, path)
    for e in range(epochs):
        ops.train_epoch(geom, net, img_d, msb_d, torch.from_numpy(perm).to(dev), bs, p, m, v, e * steps, 1e-3, losses, path=path, ws=ws)
    return [t.cpu().numpy() for t in (p, m, v, losses)]


def add_train(family, path, shape, bc, act, bs, n, alone):
    C, H, W, K, D, nl, flags = shape

    @case("lbdrn_train_epoch", family + ("_alone" if alone else ""))
    def _():
        cfg, img, msb, lab, mx, F, p0, perm, net = train_inputs(shape, bc, act, n)
        word = path | (_lib.TRAIN_ALONE if alone else 0)

        def run(dev, fill):
            A = Arena(dev)
            fit = Fit(A, dev, fill, shape, cfg, img, msb, mx, p0, perm, net, bs)
            fit.prepare(dev, path)
            for e in range(2):
                fit.epoch(dev, e, word)
            A.check()
            return fit.outs()

        def check(dev, outs):
            steps = (n + bs - 1) // bs
            assert np.isfinite(outs["params"]).all() and np.abs(outs["exp_avg"]).max() > 0
            if path == GEN:   # the oracle, step by step, at test_mfma_epoch_matches_generic_and_oracle's bounds (bc = 64, relative colours)
                feats = O.features(msb, D, ocfg_of(cfg), mx)
                po, mo, vo, lo = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), []
                with O.hidden_activation(act):
                    for s in range(2 * steps):
                        b = perm[(s % steps) * bs:(s % steps + 1) * bs]
                        l, _ = O.train_step(po, mo, vo, F, bc, C, nl, feats[b], lab[b], 1e-3, s + 1)
                        lo.append(l)
                np.testing.assert_allclose(outs["losses"], np.array(lo[steps:]), rtol=1e-5)
                assert np.linalg.norm(outs["params"] - po) <= 2e-5 * np.linalg.norm(po)
                assert np.abs(outs["exp_avg"] - mo).max() <= 2e-5 * np.abs(mo).max()
                assert np.abs(outs["exp_avg_sq"] - vo).max() <= 5e-5 * np.abs(vo).max()
                return
            # the fused steps against the generic path, at the bounds the fuzzes hold several ragged steps to
            # (test_train_fuzz_mfma_matches_generic / test_wide_window_fuzz at bc = 64, test_wide_train_fuzz_split_step_matches_generic above)
            pg, mg, vg, lg = epochs_through_ops(dev, shape, cfg, img, msb, mx, p0, perm, net, bs, GEN)
            np.testing.assert_allclose(outs["losses"], lg, rtol=5e-5 if bc == 64 else 1e-4)
            if bc == 64:
                assert np.linalg.norm(outs["params"] - pg) <= 0.01 * 1e-3 * (2 * steps) * np.sqrt(len(pg))
        return run, check


for _fam, _path, _shape, _bc, _act, _bs, _n in TRAIN_SHAPES:
    for _alone in ((False,) if _path == GEN else (False, True)):
        add_train(_fam, _path, _shape, _bc, _act, _bs, _n, _alone)


def add_train_group(family, shape, bc, act, bs, n):
    @case("lbdrn_train_epoch_group", family + "_group_of_2")
    def _():
        ins = [train_inputs(shape, bc, act, n, seed=k) for k in range(2)]
        net = ins[0][8]

        def run(dev, fill):
            A = Arena(dev)
            fits = [Fit(A, dev, fill, shape, i[0], i[1], i[2], i[4], ins[0][6], i[7], net, bs, tag=str(k)) for k, i in enumerate(ins)]
            for f in fits:
                f.prepare(dev, MFMA)
            arr = lambda bufs: (ctypes.c_void_p * 2)(*[b.data_ptr() for b in bufs])
            garr = (ctypes.POINTER(_lib.Geom) * 2)(*[ctypes.pointer(f.geom.c) for f in fits])
            for e in range(2):
                ok(call(dev, L().lbdrn_train_epoch_group, 2, ctypes.cast(garr, ctypes.c_void_p), byref(net),
                        arr([f.img for f in fits]), arr([f.msb for f in fits]), arr([f.perm for f in fits]), fits[0].n, bs,
                        arr([f.p for f in fits]), arr([f.m for f in fits]), arr([f.v for f in fits]), e * fits[0].steps, 1e-3,
                        arr([f.losses for f in fits]), arr([f.ws for f in fits]), fits[0].nws, MFMA))
            A.check()
            outs = {}
            for k, f in enumerate(fits):
                outs.update(f.outs(str(k)))
            return outs

        def check(dev, outs):   # lbdrn_hip.h: the results of `count` calls of lbdrn_train_epoch, bit for bit
            for k, i in enumerate(ins):
                p, m, v, l = epochs_through_ops(dev, shape, i[0], i[1], i[2], i[4], ins[0][6], i[7], net, bs, MFMA)
                for name, want in (("params", p), ("exp_avg", m), ("exp_avg_sq", v), ("losses", l)):
                    assert bits_equal(outs[name + str(k)], want), (k, name)
            assert not bits_equal(outs["params0"], outs["params1"])     # two different images
        return run, check


add_train_group("k_train_stream_LQ48", (8, 40, 52, 5, 2, 2, REL), 64, "sine", 512, 1025)
add_train_group("k_train_split_wide_window_C8", (8, 12, 15, 5, 3, 2, REL), 64, "sine", 33, 67)


# =============================================================== a4: lbdrn_randperm

def run_randperm(dev, A, fill, seeds, n, ws=None):
    count = len(seeds)
    perm = A.buf(count * n * 8, fill, name=f"perm_n{n}")
    nws = L().lbdrn_randperm_workspace(n, count)
    if ws is None:
        ws = A.buf(nws, fill, name="workspace")
    assert 0 < nws <= ws.nbytes
    arr = (ctypes.c_uint64 * count)(*seeds)
    ok(call(dev, L().lbdrn_randperm, arr, count, n, perm.ptr, ws.ptr, nws))
    return perm.numpy(np.int64).reshape(count, n)


def torch_randperm(seed, n):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g).numpy()


def add_randperm(n, count, family):
    @case("lbdrn_randperm", f"{family}_n{n}_count{count}")
    def _():
        seeds = [19920517, 3, 2 ** 63 - 1][:count]

        def run(dev, fill):
            A = Arena(dev)
            perm = run_randperm(dev, A, fill, seeds, n)
            A.check()
            return {"perm": perm}

        def check(dev, outs):
            for c, seed in enumerate(seeds):
                assert np.array_equal(outs["perm"][c], torch_randperm(seed, n)), (seed, n)
        return run, check


for _count in (1, 3):
    add_randperm(1000, _count, "one_segment_linked_lists")                       # below one segment, the memory-side path
    add_randperm(159746, _count, "two_segments_partitioned")                     # 159,745 draws: one word into the second segment


# =============================================================== the LBB2 plane codec

PLANE_SHAPES = [("noise_16_bit", lambda: np.random.default_rng(0).integers(0, 65536, (2, 129, 67)).astype(np.uint16)),
                ("one_column", lambda: np.random.default_rng(1).integers(0, 300, (2, 130, 1)).astype(np.uint16)),
                ("synthetic_msb", lambda: (synthetic_tile(4, 2, 140, 100) >> 4).astype(np.uint16))]


def run_plane_encode(dev, A, fill, x):
    C, H, W = x.shape
    planes = A.const(x, "planes")
    bound = L().lbdrn_plane_bound(C, H, W)
    body, nbytes = A.buf(bound, fill, name="body"), A.buf(8, fill, name="body_bytes")
    nws = L().lbdrn_plane_workspace(C, H, W)
    ws = A.buf(nws, fill, name="workspace")
    ok(call(dev, L().lbdrn_plane_encode, planes.ptr, C, H, W, body.ptr, bound, nbytes.ptr, ws.ptr, nws))
    n = int(nbytes.numpy(np.uint64)[0])
    assert n <= bound, (n, bound)
    return body.numpy(np.uint8)[:n]


def add_plane_encode(name, make):
    @case("lbdrn_plane_encode", name)
    def _():
        x = make()

        def run(dev, fill):
            A = Arena(dev)
            body = run_plane_encode(dev, A, fill, x)
            A.check()
            return {"body": body}

        def check(dev, outs):
            assert outs["body"].tobytes() == _oracle_body(x)
        return run, check


def run_plane_decode(dev, A, fill, body, C, H, W):
    """-> (rc, status, planes); the body is a const input of exactly its length"""
    raw = A.const(np.frombuffer(bytes(body), np.uint8), "body")
    planes = A.buf(C * H * W * 2, fill, name="planes")
    status = A.buf(4, fill, name="status")
    nws = L().lbdrn_plane_workspace(C, H, W)
    ws = A.buf(nws, fill, name="workspace")
    rc = call(dev, L().lbdrn_plane_decode, raw.ptr, len(body), C, H, W, planes.ptr, status.ptr, ws.ptr, nws)
    return rc, status, planes


def add_plane_decode(name, make):
    @case("lbdrn_plane_decode", name)
    def _():
        x = make()
        body = _oracle_body(x)

        def run(dev, fill):
            A = Arena(dev)
            rc, status, planes = run_plane_decode(dev, A, fill, body, *x.shape)
            ok(rc)
            A.check()
            return {"planes": planes.numpy(np.uint16), "status": status.numpy(np.int32)}

        def check(dev, outs):
            assert int(outs["status"][0]) == 0 and np.array_equal(outs["planes"], x.reshape(-1))
        return run, check


def damaged_bodies():
    """the damaged streams of test_damaged_streams_are_rejected_not_trusted, from the oracle's body of the same planes;
    (name, body, must_be_rejected)"""
    x = (synthetic_tile(4, 2, 140, 100) >> 4).astype(np.uint16)
    C, H, W = x.shape
    body = _oracle_body(x)
    ns = C * ((W + 63) // 64)
    yield "cannot_hold_the_counts", body[:8], True
    yield "counts_promise_more_words", body[:-40], True
    bad = bytearray(body)
    struct.pack_into("<I", bad, 0, struct.unpack_from("<I", bad, 0)[0] - 3)
    yield "a_strip_claims_fewer_words", bytes(bad), True
    bad = bytearray(body)
    struct.pack_into("<I", bad, 4 * ns, 0x77)
    yield "k0_out_of_range", bytes(bad), True
    rng = np.random.default_rng(1)
    for k in range(4):   # (random words can form a consistent stream: the existing test accepts either outcome, so does this one)
        bad = bytearray(body)
        bad[4 * ns + 8:] = rng.integers(0, 256, len(bad) - 4 * ns - 8, dtype=np.uint8).tobytes()
        yield f"noise_{k}", bytes(bad), False


def add_plane_decode_damaged(name, body, must_reject):
    @case("lbdrn_plane_decode", "damaged_" + name)
    def _():
        C, H, W = 2, 140, 100

        def run(dev, fill):
            """the header's promise: the call terminates, reports the damage (an error, or a non-zero status), and the planes --
            unspecified, not compared -- stay in bounds: the guards around planes, status and the workspace are intact"""
            A = Arena(dev)
            rc, status, planes = run_plane_decode(dev, A, fill, body, C, H, W)
            A.check()
            if must_reject:
                assert rc != 0 or int(status.numpy(np.int32)[0]) != 0, "a damaged stream was accepted"
            assert rc in (0, _lib.E_ARG), rc
            return {}

        return run, lambda dev, outs: None


for _name, _make in PLANE_SHAPES:
    add_plane_encode(_name, _make)
    add_plane_decode(_name, _make)
for _name, _body, _must in damaged_bodies():
    add_plane_decode_damaged(_name, _body, _must)


# =============================================================== the matrix

def first_difference(base, outs):
    for name in base:
        a, b = base[name], outs[name]
        if not bits_equal(a, b):
            if a.shape != b.shape:
                return f"'{name}': shapes {a.shape} and {b.shape}"
            ai, bi = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
            at = int(np.flatnonzero(ai != bi)[0]) // a.dtype.itemsize
            count = int((a.reshape(-1) != b.reshape(-1)).sum())
            return f"'{name}' differs at element {at} of {a.size} ({a.reshape(-1)[at]!r} with a zeroed buffer, {b.reshape(-1)[at]!r} now; {count} elements differ)"
    return None


@pytest.mark.parametrize("case,fill", [pytest.param(c, f, id=f"{c.id}-{fill_id(f)}") for c in CASES for f in FILLS])
def test_scratch_and_output_contents_do_not_matter_and_guards_stay(dev, case, fill):
    if fill == FILLS[0]:
        outs = case.run(dev, fill)
        _BASE[case.id] = outs
        case.check(dev, outs)
        return
    if case.id not in _BASE:       # (this fill selected alone: -k)
        _BASE[case.id] = case.run(dev, FILLS[0])
    outs = case.run(dev, fill)
    diff = first_difference(_BASE[case.id], outs)
    assert diff is None, f"{case.id}: the result depends on what the scratch / output buffers held ({fill_id(fill)}): {diff}"


def test_every_device_entry_point_of_the_header_has_a_case():
    """every function include/lbdrn_hip.h declares with a device pointer (lbdrn_jp2k_encode has its own test of this kind in
    tests/test_gpu_jp2k.py; lbdrn_train_prepare runs in front of every lbdrn_train_epoch case)"""
    covered = {c.id.split("-")[0] for c in CASES} | {"lbdrn_train_prepare", "lbdrn_jp2k_encode"}
    device_entries = {"lbdrn_split_bits", "lbdrn_labels", "lbdrn_features", "lbdrn_forward", "lbdrn_forward_tape", "lbdrn_backward",
                      "lbdrn_decode_fused", "lbdrn_eval_sse", "lbdrn_train_prepare", "lbdrn_train_epoch", "lbdrn_train_epoch_group",
                      "lbdrn_randperm", "lbdrn_plane_encode", "lbdrn_plane_decode", "lbdrn_jp2k_encode", "lbdrn_train_step"}
    host_only = {"lbdrn_last_error", "lbdrn_abi_version", "lbdrn_device_check", "lbdrn_param_count", "lbdrn_feature_dim",
                 "lbdrn_apply_instance", "lbdrn_train_group_max", "lbdrn_train_step_features", "lbdrn_train_group_size", "lbdrn_train_profile_mode",
                 "lbdrn_mt19937_jump_poly", "lbdrn_jp2k_block_count", "lbdrn_weights_encode", "lbdrn_weights_info", "lbdrn_weights_decode"}
    sizing = {n for n in _lib.SIGNATURES if n.endswith(("_workspace", "_bound", "_bytes"))}
    assert device_entries | host_only | sizing == set(_lib.SIGNATURES), set(_lib.SIGNATURES) ^ (device_entries | host_only | sizing)
    assert device_entries <= covered, device_entries - covered


# =============================================================== reuse: a large shape, then a small one, in one workspace

def test_apply_workspace_reused_for_a_smaller_shape(dev):
    """bc = 256 on 8 x 48 x 64, then bc = 64 on 4 x 30 x 41, in the workspace the first left behind (sized for the first,
    not refilled): the second raster, sigmoid outputs and sum equal those from a fresh workspace, on either path"""
    big = apply_inputs(256, (8, 48, 64))
    small = apply_inputs(64, (4, 30, 41))

    def run(A, ins, shape, path, ws):
        cfg, img, msb_np, lab, mx, F, pn, net = ins
        C, H, W = shape
        geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, cfg, dev)
        src, msb, p = A.const(img, "img"), A.const(msb_np, "msb"), A.const(pn, "params")
        out, y, sse = A.buf(C * H * W * 2, 0xA5, name="out"), A.buf(H * W * C * 4, 0xA5, name="y_out"), A.buf(8, 0xA5, name="sse")
        nws = L().lbdrn_apply_workspace(byref(geom.c), byref(net))
        ws = ws if ws is not None else A.buf(nws, 0x00, name="fresh workspace")
        assert nws <= ws.nbytes
        ok(call(dev, L().lbdrn_decode_fused, byref(geom.c), byref(net), msb.ptr, p.ptr, out.ptr, y.ptr, ws.ptr, nws, path))
        ok(call(dev, L().lbdrn_eval_sse, byref(geom.c), byref(net), src.ptr, msb.ptr, p.ptr, sse.ptr, ws.ptr, nws, path))
        A.check()
        return {"out": out.numpy(np.uint16), "y": y.numpy(np.float32), "sse": sse.numpy(np.float64)}, nws

    for path in (MFMA, GEN):
        A = Arena(dev)
        cfg, img, msb_np, lab, mx, F, pn, net = big
        nbig = L().lbdrn_apply_workspace(byref(ops.FeatureGeometry(8, 48, 64, 5, 2, mx, cfg, dev).c), byref(net))
        shared = A.buf(nbig, 0xFF, name="shared workspace")
        first, _ = run(A, big, (8, 48, 64), path, shared)
        out_o = O.decode(msb_np, 5, 2, ocfg_of(cfg), pn, 256, 2, mx)
        assert np.array_equal(first["out"], out_o.reshape(-1))
        second, nsmall = run(A, small, (4, 30, 41), path, shared)
        assert nsmall < nbig
        fresh, _ = run(Arena(dev), small, (4, 30, 41), path, None)
        assert first_difference(fresh, second) is None, (path, first_difference(fresh, second))
        assert np.array_equal(fresh["out"], O.decode(small[2], 5, 2, ocfg_of(small[0]), small[6], 64, 2, small[4]).reshape(-1))


@pytest.mark.parametrize("path", (MFMA, GEN), ids=("fused", "generic"))
def test_training_workspace_reused_for_a_smaller_image(dev, path):
    """prepare and step image A (8 x 40 x 52), then prepare and step image B (4 x 30 x 41) in the same buffer: B's parameters,
    moments and losses equal those from a fresh workspace"""
    sa, sb = (8, 40, 52, 5, 2, 2, REL), (4, 30, 41, 5, 2, 2, REL)
    ia, ib = train_inputs(sa, 64, "sine", 1025), train_inputs(sb, 64, "sine", 617)

    def fit(A, shape, ins, bs, ws):
        cfg, img, msb, lab, mx, F, p0, perm, net = ins
        f = Fit(A, dev, 0xA5, shape, cfg, img, msb, mx, p0, perm, net, bs, ws=ws)
        f.prepare(dev, path)
        for e in range(2):
            f.epoch(dev, e, path)
        A.check()
        return f

    A = Arena(dev)
    first = fit(A, sa, ia, 512, None)
    second = fit(A, sb, ib, 300, first.ws)
    assert second.nws < first.nws
    fresh = fit(Arena(dev), sb, ib, 300, None)
    assert first_difference(fresh.outs(), second.outs()) is None, first_difference(fresh.outs(), second.outs())
    assert np.isfinite(second.outs()["params"]).all() and np.abs(second.outs()["exp_avg"]).max() > 0


def test_randperm_workspace_reused_for_a_shorter_permutation(dev):
    """159,746 elements (partitioned, two segments), then 1000 and 40,000 in the same workspace: torch.randperm's, each"""
    A = Arena(dev)
    seeds = [19920517, 3]
    ws = A.buf(L().lbdrn_randperm_workspace(159746, 2), 0xA5, name="shared workspace")
    for n in (159746, 1000, 40000, 159746):
        got = run_randperm(dev, A, 0xA5, seeds, n, ws=ws)
        A.check()
        for c, seed in enumerate(seeds):
            assert np.array_equal(got[c], torch_randperm(seed, n)), (seed, n)


# =============================================================== refusals: one byte less than the sizing function returned

def refusal_cases():
    """(id, call(dev, A, short) -> (rc, [output buffers])): every entry point that takes a size, given `short` bytes less.
    The size checks stand in front of every launch (csrc/cabi.hip for the apply and training entry points, the first lines of
    generic_forward / generic_forward_tape / generic_backward / generic_train_step, randperm_batch, plane_encode /
    plane_decode): a refused call launches nothing, so no kernel ever runs on a short buffer here."""
    bc, B, act, F, C, nl = 65, 65, "sine", 37, 5, 2
    pn, x, t, net = net_inputs(bc, B, act, F, C, nl)
    NP = pn.size

    def forward(dev, A, short):
        p, xd, y = A.const(pn), A.const(x), A.buf(B * C * 4, 0xA5, name="y")
        nws = L().lbdrn_forward_workspace(byref(net), B)
        ws = A.buf(nws, 0xA5, name="workspace")
        return call(dev, L().lbdrn_forward, byref(net), p.ptr, xd.ptr, B, y.ptr, ws.ptr, nws - short), [y, ws]
    yield "lbdrn_forward", forward

    def forward_tape(dev, A, short):
        p, xd, y = A.const(pn), A.const(x), A.buf(B * C * 4, 0xA5, name="y")
        nt = L().lbdrn_tape_bytes(byref(net), B)
        tape = A.buf(nt, 0xA5, name="tape")
        return call(dev, L().lbdrn_forward_tape, byref(net), p.ptr, xd.ptr, B, y.ptr, tape.ptr, nt - short), [y, tape]
    yield "lbdrn_forward_tape", forward_tape

    def backward(which):
        def f(dev, A, short):
            p, xd, y, dy = A.const(pn), A.const(x), A.const(t), A.const(t)
            nt, nws = L().lbdrn_tape_bytes(byref(net), B), L().lbdrn_backward_workspace(byref(net), B)
            tape = A.const(np.zeros(nt, np.uint8), "tape")
            grads, dx, ws = A.buf(NP * 4, 0xA5, name="grads"), A.buf(B * F * 4, 0xA5, name="dx"), A.buf(nws, 0xA5, name="workspace")
            return call(dev, L().lbdrn_backward, byref(net), p.ptr, xd.ptr, B, tape.ptr, nt - (short if which == "tape" else 0),
                        y.ptr, dy.ptr, grads.ptr, dx.ptr, ws.ptr, nws - (short if which == "workspace" else 0)), [grads, dx, ws]
        return f
    yield "lbdrn_backward-short_tape", backward("tape")
    yield "lbdrn_backward-short_workspace", backward("workspace")

    def train_step(dev, A, short):
        xd, td = A.const(x), A.const(t)
        if short:                                      # (a refused call leaves the optimiser state alone too)
            p, m, v = A.const(pn, "params"), A.const(np.zeros_like(pn), "exp_avg"), A.const(np.zeros_like(pn), "exp_avg_sq")
        else:
            p, m, v = A.buf(NP * 4, 0, name="params").write(pn), A.buf(NP * 4, 0, name="exp_avg"), A.buf(NP * 4, 0, name="exp_avg_sq")
        loss, grads = A.buf(4, 0xA5, name="loss"), A.buf(NP * 4, 0xA5, name="grads")
        nws = train_step_workspace(net, B)
        ws = A.buf(nws, 0xA5, name="workspace")
        return call(dev, L().lbdrn_train_step, byref(net), xd.ptr, td.ptr, B, p.ptr, m.ptr, v.ptr, 1, 1e-3, 1, loss.ptr, grads.ptr,
                    ws.ptr, nws - short), [loss, grads, ws]
    yield "lbdrn_train_step", train_step

    for family, path, abc, shape in (("generic", GEN, 32, (3, 17, 37)), ("k_apply_mfma", MFMA, 64, (4, 130, 70)), ("k_apply_wide", MFMA, 256, (8, 48, 64))):
        cfg, img, msb_np, lab, mx, aF, apn, anet = apply_inputs(abc, shape)
        aC, aH, aW = shape

        def decode(dev, A, short, cfg=cfg, msb_np=msb_np, mx=mx, apn=apn, anet=anet, aC=aC, aH=aH, aW=aW, path=path):
            geom = ops.FeatureGeometry(aC, aH, aW, 5, 2, mx, cfg, dev)
            msb, p = A.const(msb_np), A.const(apn)
            out, y = A.buf(aC * aH * aW * 2, 0xA5, name="out"), A.buf(aH * aW * aC * 4, 0xA5, name="y_out")
            nws = L().lbdrn_apply_workspace(byref(geom.c), byref(anet))
            ws = A.buf(nws, 0xA5, name="workspace")
            return call(dev, L().lbdrn_decode_fused, byref(geom.c), byref(anet), msb.ptr, p.ptr, out.ptr, y.ptr, ws.ptr, nws - short, path), [out, y, ws]
        yield f"lbdrn_decode_fused-{family}", decode

        def evaluate(dev, A, short, cfg=cfg, img=img, msb_np=msb_np, mx=mx, apn=apn, anet=anet, aC=aC, aH=aH, aW=aW, path=path):
            geom = ops.FeatureGeometry(aC, aH, aW, 5, 2, mx, cfg, dev)
            src, msb, p = A.const(img), A.const(msb_np), A.const(apn)
            sse = A.buf(8, 0xA5, name="sse")
            nws = L().lbdrn_apply_workspace(byref(geom.c), byref(anet))
            ws = A.buf(nws, 0xA5, name="workspace")
            return call(dev, L().lbdrn_eval_sse, byref(geom.c), byref(anet), src.ptr, msb.ptr, p.ptr, sse.ptr, ws.ptr, nws - short, path), [sse, ws]
        yield f"lbdrn_eval_sse-{family}", evaluate

    for family, path, shape, tbc, bs, n in (("generic", GEN, (4, 30, 41, 5, 2, 2, REL), 64, 300, 617),
                                            ("k_train_stream", MFMA, (8, 40, 52, 5, 2, 2, REL), 64, 512, 1025),
                                            ("k_train_split_wide_window", MFMA, (8, 12, 15, 5, 3, 2, REL), 64, 33, 67),
                                            ("k_train_half", MFMA, (8, 40, 52, 5, 2, 2, REL), 256, 352, 721)):
        ins = train_inputs(shape, tbc, "sine", n)

        def prepare(dev, A, short, ins=ins, shape=shape, bs=bs, path=path):
            cfg, img, msb, lab, mx, tF, p0, perm, tnet = ins
            f = Fit(A, dev, 0xA5, shape, cfg, img, msb, mx, p0, perm, tnet, bs)
            return call(dev, L().lbdrn_train_prepare, byref(f.geom.c), byref(tnet), f.img.ptr, f.msb.ptr, bs, f.ws.ptr, f.nws - short, path), [f.ws]
        yield f"lbdrn_train_prepare-{family}", prepare

        def epoch(dev, A, short, ins=ins, shape=shape, bs=bs, path=path):
            cfg, img, msb, lab, mx, tF, p0, perm, tnet = ins
            f = Fit(A, dev, 0xA5, shape, cfg, img, msb, mx, p0, perm, tnet, bs)
            if not short:
                f.prepare(dev, path)
            state = [A.const(p0, "params"), A.const(np.zeros_like(p0), "exp_avg"), A.const(np.zeros_like(p0), "exp_avg_sq")]
            if not short:          # (the complete call may update its state: hand it the fit's own)
                state = [f.p, f.m, f.v]
            return call(dev, L().lbdrn_train_epoch, byref(f.geom.c), byref(tnet), f.img.ptr, f.msb.ptr, f.perm.ptr, f.n, bs, state[0].ptr,
                        state[1].ptr, state[2].ptr, 0, 1e-3, f.losses.ptr, f.ws.ptr, f.nws - short, path), [f.losses, f.ws]
        yield f"lbdrn_train_epoch-{family}", epoch

    gins = [train_inputs((8, 40, 52, 5, 2, 2, REL), 64, "sine", 1025, seed=k) for k in range(2)]

    def group(dev, A, short):
        shape, bs = (8, 40, 52, 5, 2, 2, REL), 512
        fits = [Fit(A, dev, 0xA5, shape, i[0], i[1], i[2], i[4], gins[0][6], i[7], gins[0][8], bs, tag=str(k)) for k, i in enumerate(gins)]
        if not short:
            for f in fits:
                f.prepare(dev, MFMA)
        state = [[f.p, f.m, f.v] if not short else [A.const(gins[0][6]), A.const(np.zeros_like(gins[0][6])), A.const(np.zeros_like(gins[0][6]))] for f in fits]
        arr = lambda bufs: (ctypes.c_void_p * 2)(*[b.data_ptr() for b in bufs])
        garr = (ctypes.POINTER(_lib.Geom) * 2)(*[ctypes.pointer(f.geom.c) for f in fits])
        rc = call(dev, L().lbdrn_train_epoch_group, 2, ctypes.cast(garr, ctypes.c_void_p), byref(gins[0][8]), arr([f.img for f in fits]),
                  arr([f.msb for f in fits]), arr([f.perm for f in fits]), fits[0].n, bs, arr([s[0] for s in state]), arr([s[1] for s in state]),
                  arr([s[2] for s in state]), 0, 1e-3, arr([f.losses for f in fits]), arr([f.ws for f in fits]), fits[0].nws - short, MFMA)
        return rc, [f.losses for f in fits] + [f.ws for f in fits]
    yield "lbdrn_train_epoch_group-k_train_stream", group

    for n in (1000, 159746):
        def randperm(dev, A, short, n=n):
            perm = A.buf(2 * n * 8, 0xA5, name="perm")
            nws = L().lbdrn_randperm_workspace(n, 2)
            ws = A.buf(nws, 0xA5, name="workspace")
            return call(dev, L().lbdrn_randperm, (ctypes.c_uint64 * 2)(5, 6), 2, n, perm.ptr, ws.ptr, nws - short), [perm, ws]
        yield f"lbdrn_randperm-n{n}", randperm

    xp = (synthetic_tile(4, 2, 140, 100) >> 4).astype(np.uint16)

    def plane_encode(which):
        def f(dev, A, short):
            planes = A.const(xp)
            bound, nws = L().lbdrn_plane_bound(2, 140, 100), L().lbdrn_plane_workspace(2, 140, 100)
            body, nbytes, ws = A.buf(bound, 0xA5, name="body"), A.buf(8, 0xA5, name="body_bytes"), A.buf(nws, 0xA5, name="workspace")
            return call(dev, L().lbdrn_plane_encode, planes.ptr, 2, 140, 100, body.ptr, bound - (short if which == "body" else 0), nbytes.ptr,
                        ws.ptr, nws - (short if which == "workspace" else 0)), [body, nbytes, ws]
        return f
    yield "lbdrn_plane_encode-short_workspace", plane_encode("workspace")
    yield "lbdrn_plane_encode-short_body", plane_encode("body")

    def plane_decode(dev, A, short):
        body = _oracle_body(xp)
        rc, status, planes = run_plane_decode(dev, A, 0xA5, body, 2, 140, 100) if not short else (None, None, None)
        if short:
            raw = A.const(np.frombuffer(body, np.uint8), "body")
            planes, status = A.buf(xp.nbytes, 0xA5, name="planes"), A.buf(4, 0xA5, name="status")
            nws = L().lbdrn_plane_workspace(2, 140, 100)
            ws = A.buf(nws, 0xA5, name="workspace")
            rc = call(dev, L().lbdrn_plane_decode, raw.ptr, len(body), 2, 140, 100, planes.ptr, status.ptr, ws.ptr, nws - 1)
            return rc, [planes, status, ws]
        return rc, [planes, status]
    yield "lbdrn_plane_decode", plane_decode


_REFUSALS = list(refusal_cases())


@pytest.mark.parametrize("name,fn", _REFUSALS, ids=[n for n, _ in _REFUSALS])
def test_one_byte_short_is_refused_and_nothing_is_written(dev, name, fn):
    """With exactly the size the sizing function returned the call succeeds; with one byte less it answers
    LBDRN_E_WORKSPACE, names the sizes, and leaves every output, the workspace and every guard as they were."""
    A = Arena(dev)
    rc, _ = fn(dev, A, 0)
    ok(rc)
    A.check()
    A = Arena(dev)
    rc, untouched = fn(dev, A, 1)
    assert rc == _lib.E_WORKSPACE, (rc, (L().lbdrn_last_error() or b"").decode())
    assert b"too small" in (L().lbdrn_last_error() or b"")
    A.check()
    for b in untouched:
        assert bool((b.t == 0xA5).all()), f"{name}: '{b.name}' was written by a refused call"
