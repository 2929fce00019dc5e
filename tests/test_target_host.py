"""encode.py --target-psnr / --target-bpsp on the host: lbdrn_hip.target.choose on hand-made tables, the parser errors (before
any device work), the LBDRN_EVAL_DECODED flag in the header and the binding, and -- through ctypes, without a device, ahead of
LBDRN_E_DEVICE -- the flag rules of lbdrn_eval_sse and lbdrn_apply_instance.  The device side: tests/test_gpu_eval_decoded.py
and tests/test_gpu_target.py."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
for p in (PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lbdrn_hip.target import Candidate, TargetNotMet, choose  # noqa: E402

N = 1000      # samples of the hand-made scenes


def _c(K, nbytes, sse):
    return Candidate(K, nbytes, sse, N)


# ---------------------------------------------------------------- target.choose

def test_candidate_figures():
    c = _c(4, 250, 4000)
    assert c.mse == 4.0 and c.bpsp == 2.0 and c.psnr() == 10 * math.log10(10000.0 ** 2 / 4.0)
    assert c.psnr(255.0) == 10 * math.log10(255.0 ** 2 / 4.0)
    assert _c(1, 900, 0).psnr() == math.inf and _c(1, 900, 0).mse == 0.0


def test_psnr_target_takes_the_smallest_eligible_file():
    # not monotone: K = 4 is larger AND worse than K = 3, K = 6 is the smallest file and the worst
    table = [_c(2, 700, 100), _c(3, 500, 400), _c(4, 600, 900), _c(5, 450, 1600), _c(6, 300, 90000)]
    psnr = {c.K: c.psnr() for c in table}
    assert psnr[2] > psnr[3] > psnr[4] > psnr[5] > psnr[6]
    assert choose(table, psnr=0.0).K == 6
    assert choose(table, psnr=psnr[5]).K == 5                           # the bound itself is met
    assert choose(table, psnr=(psnr[5] + psnr[4]) / 2).K == 3           # K = 4 is eligible too, and larger
    assert choose(table, psnr=(psnr[3] + psnr[2]) / 2).K == 2
    assert choose(reversed(table), psnr=(psnr[5] + psnr[4]) / 2).K == 3       # the order of the table does not matter
    with pytest.raises(TargetNotMet) as e:
        choose(table, psnr=psnr[2] + 0.001)
    assert e.value.table == table and "psnr >=" in str(e.value)
    # a tie on the file size: the larger K
    tie = [_c(3, 500, 100), _c(4, 500, 200), _c(5, 500, 300), _c(6, 400, 10 ** 9)]
    assert choose(tie, psnr=_c(0, 0, 300).psnr()).K == 5
    assert choose(tie, psnr=_c(0, 0, 250).psnr()).K == 4
    # sse == 0 counts as +inf: it meets any target, and loses to a smaller eligible file
    lossless = [_c(1, 900, 0), _c(2, 800, 10)]
    assert choose(lossless, psnr=1e9).K == 1 and choose(lossless, psnr=math.inf).K == 1
    assert choose(lossless, psnr=_c(0, 0, 10).psnr()).K == 2
    assert choose(lossless, psnr=80.0, peak=1.0).K == 1                 # the peak is the caller's


def test_bpsp_target_takes_the_least_distortion():
    table = [_c(2, 700, 100), _c(3, 500, 400), _c(4, 600, 300), _c(5, 450, 1600), _c(6, 300, 90000)]      # bpsp 5.6 4.0 4.8 3.6 2.4
    assert choose(table, bpsp=100.0).K == 2
    assert choose(table, bpsp=5.0).K == 4                               # not monotone: the larger K is the better point here
    assert choose(table, bpsp=4.8).K == 4                               # the bound itself is met
    assert choose(table, bpsp=4.5).K == 3
    assert choose(table, bpsp=3.0).K == 6
    with pytest.raises(TargetNotMet) as e:
        choose(table, bpsp=2.39)
    assert e.value.table == table and "bpsp <=" in str(e.value)
    # a tie on sse: the smaller file
    tie = [_c(3, 500, 400), _c(4, 450, 400), _c(5, 480, 400), _c(6, 100, 401)]
    assert choose(tie, bpsp=100.0).K == 4
    assert choose([_c(1, 900, 0), _c(2, 800, 0), _c(3, 10, 1)], bpsp=100.0).K == 2
    for bad in ({}, {"psnr": 1.0, "bpsp": 1.0}):
        with pytest.raises(ValueError):
            choose(table, **bad)
    with pytest.raises(TargetNotMet):
        choose([], psnr=0.0)


# ---------------------------------------------------------------- the command line

ARGS = ["-e", "2", "-bs", "64"]


def test_parser_errors_come_before_any_device_work(tmp_path, monkeypatch, capsys):
    import encode
    from lbdrn_hip import shard

    def never(*a, **k):
        raise AssertionError("device work was started")
    for name in ("train_tiles", "train_tiles_at", "report_and_pack", "tile_distortion", "nodata_mask", "main_target"):
        monkeypatch.setattr(encode, name, never)
    monkeypatch.setattr(shard, "init_host_group", never)
    monkeypatch.setattr(encode.raster_io, "read_raster", never)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    npy = str(tmp_path / "scene.npy")
    np.save(npy, np.zeros((2, 8, 8), np.uint16))
    out = tmp_path / "out"
    cases = [
        (["--target-psnr", "60", "--target-bpsp", "2"], "not allowed with"),
        (["--target-psnr", "60", "--max-error", "2"], "--max-error"),
        (["--target-bpsp", "2.5", "--max-error", "0"], "--max-error"),
        (["--target-psnr", "60", "--nodata", "0"], "--nodata"),
        (["--target-bpsp", "2.5", "--nodata", "tag"], "--nodata"),
        (["--target-psnr", "60", "--target-k", "0", "4"], "--target-k"),
        (["--target-psnr", "60", "--target-k", "3", "12"], "--target-k"),
        (["--target-psnr", "60", "--target-k", "5", "4"], "--target-k"),
        (["--target-k", "3", "6"], "--target-k"),
        (["--target-peak", "255"], "--target-peak"),
        (["--target-psnr", "60", "--target-peak", "0"], "--target-peak"),
        (["--report-distortion", "--max-error", "2"], "--max-error"),
        (["--report-distortion", "--nodata", "0"], "--nodata"),
    ]
    for extra, word in cases:
        with pytest.raises(SystemExit) as e:
            encode.main(["-i", npy, "-o", str(out)] + extra + ARGS, shard_tiles=False)
        assert e.value.code == 2 and word in capsys.readouterr().err and not out.exists(), extra
    # a target under a tile-sharded launch: asked for, or found in the environment
    with pytest.raises(SystemExit) as e:
        encode.main(["-i", npy, "-o", str(out), "--target-psnr", "60"] + ARGS, shard_tiles=True)
    assert e.value.code == 2 and "tile-sharded" in capsys.readouterr().err and not out.exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        encode.main(["-i", npy, "-o", str(out), "--target-bpsp", "2"] + ARGS)
    assert e.value.code == 2 and "tile-sharded" in capsys.readouterr().err and not out.exists()


def test_the_request_and_what_a_run_without_it_parses_to():
    import encode
    parser = encode.build_parser()
    plain = parser.parse_args(["-i", "a.tif"])
    assert not any(hasattr(plain, name) for name in encode.TARGET_ARGS + ("report_distortion",))      # the `Namespace` record stays
    assert encode.target_request(parser, plain) is None
    a = parser.parse_args(["-i", "a.tif", "--target-psnr", "60"])
    assert encode.target_request(parser, a) == (60.0, None, [1, 2, 3, 4, 5, 6, 7, 8], 10000.0)
    a = parser.parse_args(["-i", "a.tif", "--target-bpsp", "2.5", "--target-k", "3", "6", "--target-peak", "4095", "-K", "9"])
    assert encode.target_request(parser, a) == (None, 2.5, [3, 4, 5, 6], 4095.0)
    a = parser.parse_args(["-i", "a.tif", "--target-psnr", "0", "--target-k", "11", "11"])
    assert encode.target_request(parser, a)[2] == [11]
    a = parser.parse_args(["-i", "a.tif", "--report-distortion", "--target-peak", "255"])
    assert encode.target_request(parser, a) is None and a.report_distortion is True
    from lbdrn_hip.target import Candidate as C
    c = C(5, 1234, 4000, 1000)
    assert encode.candidate_record(c, 10000.0) == f"Candidate K=5: bytes=1234 bpsp={1234 * 8 / 1000!r} sse=4000 mse=4.0 psnr={c.psnr()!r}"
    assert encode.distortion_record(c, 10000.0) == f"Closed-loop: sse=4000 mse=4.0 psnr={c.psnr()!r}"
    assert encode.distortion_record(C(5, 1, 0, 10), 10000.0) == "Closed-loop: sse=0 mse=0.0 psnr=inf"


# ---------------------------------------------------------------- the flag

def test_the_flag_is_in_the_header_and_the_binding():
    from lbdrn_hip import _lib, codec, ops
    with open(os.path.join(ROOT, "include", "lbdrn_hip.h")) as f:
        text = f.read()
    (value,) = re.findall(r"^#define LBDRN_EVAL_DECODED (0x[0-9A-Fa-f]+)$", text, re.M)
    assert int(value, 16) == _lib.EVAL_DECODED == 0x8000
    assert re.search(r"^#define LBDRN_ABI_VERSION 2$", text, re.M)      # additive
    # disjoint from every other flag of the `path` word, as the header defines them, and from the path values
    others = {name: int(v, 16) for name, v in re.findall(r"^#define (LBDRN_(?:EVAL|APPLY|TRAIN)_[A-Z0-9]+) (0x[0-9A-Fa-f]+)", text, re.M)
              if name != "LBDRN_EVAL_DECODED"}
    assert {"LBDRN_EVAL_BACKGROUND", "LBDRN_EVAL_FAST", "LBDRN_EVAL_X16", "LBDRN_EVAL_VALID", "LBDRN_APPLY_DECODE", "LBDRN_TRAIN_ALONE"} <= set(others)
    assert all(_lib.EVAL_DECODED & v == 0 for v in others.values()), others
    assert all(_lib.EVAL_DECODED & v == 0 for v in (_lib.PATH_AUTO, _lib.PATH_GENERIC, _lib.PATH_MFMA, _lib.EVAL_BACKGROUND, _lib.EVAL_FAST,
                                                    _lib.EVAL_X16, _lib.EVAL_VALID, _lib.APPLY_DECODE, _lib.TRAIN_ALONE))
    assert inspect.signature(ops.eval_sse).parameters["decoded"].default is False
    assert list(inspect.signature(codec.closed_loop_sse).parameters)[:7] == ["fit_result", "img", "nn_payload", "K", "D", "base_channel", "num_layers"]


SHAPES = ((4, 30, 41, 64, 2), (8, 48, 130, 32, 1), (4, 30, 41, 256, 2), (4, 30, 41, 128, 2))


def test_flag_rules_are_checked_before_the_device():
    """The pointers are never followed: every call here ends at the argument checks, which come before the device is looked
    for (a machine without one answers LBDRN_E_DEVICE only behind them) and before any launch."""
    from lbdrn_hip import _lib
    lib = _lib.lib()
    DEC, FAST, X16, BG, VALID = _lib.EVAL_DECODED, _lib.EVAL_FAST, _lib.EVAL_X16, _lib.EVAL_BACKGROUND, _lib.EVAL_VALID
    fake = ctypes.c_void_p(4096)
    for (C, H, W, bc, nl) in SHAPES:
        net = _lib.Net(C * 25, bc, C, nl, 0)
        g = _lib.Geom(C, H, W, 5, 2, 300, 1, 1, 0, 0, None, None)
        call = lambda msb, word: lib.lbdrn_eval_sse(ctypes.byref(g), ctypes.byref(net), fake, msb, fake, fake, fake, 0, word, None)
        for path in (_lib.PATH_AUTO, _lib.PATH_GENERIC, _lib.PATH_MFMA):
            for word in (DEC | FAST, DEC | FAST | X16, DEC | X16, DEC | FAST | BG, DEC | FAST | VALID):
                assert call(fake, path | word) == _lib.E_ARG
                msg = lib.lbdrn_last_error()
                assert b"LBDRN_EVAL_DECODED" in msg and b"canonical" in msg, msg
                assert call(None, path | word) == _lib.E_ARG and b"canonical" in lib.lbdrn_last_error()      # (FAST alone may leave msb out; not here)
            for word in (DEC, DEC | BG, DEC | VALID):
                assert call(None, path | word) == _lib.E_ARG
                msg = lib.lbdrn_last_error()
                assert b"LBDRN_EVAL_DECODED" in msg and b"msb" in msg, msg
    # the flag beside an unknown path value is still an unknown path
    assert call(fake, DEC | 3) == _lib.E_ARG and b"unknown path" in lib.lbdrn_last_error()


def test_apply_instance_ignores_the_flag():
    from lbdrn_hip import _lib
    lib = _lib.lib()
    for (C, H, W, bc, nl) in SHAPES:
        net = _lib.Net(C * 25, bc, C, nl, 0)
        g = _lib.Geom(C, H, W, 5, 2, 300, 1, 1, 0, 0, None, None)
        for path in (_lib.PATH_AUTO, _lib.PATH_MFMA):
            for word in (0, _lib.EVAL_FAST, _lib.EVAL_FAST | _lib.EVAL_X16, _lib.EVAL_BACKGROUND, _lib.EVAL_VALID, _lib.APPLY_DECODE):
                got = []
                for flag in (0, _lib.EVAL_DECODED):
                    out = (ctypes.c_int32 * 8)(*([-1] * 8))
                    rc = lib.lbdrn_apply_instance(ctypes.byref(g), ctypes.byref(net), path | word | flag, out)
                    got.append((rc, list(out)))
                assert got[0] == got[1] and got[0][0] == 0 and got[0][1][0] in (1, 2), (bc, word, got)
    # a shape without a fused kernel: the same refusal with and without it
    net = _lib.Net(4 * 25, 96, 4, 2, 0)
    g = _lib.Geom(4, 30, 41, 5, 2, 300, 1, 1, 0, 0, None, None)
    out = (ctypes.c_int32 * 8)(*([-1] * 8))
    assert [lib.lbdrn_apply_instance(ctypes.byref(g), ctypes.byref(net), _lib.PATH_MFMA | f, out) for f in (0, _lib.EVAL_DECODED)] == [_lib.E_UNSUPPORTED] * 2
    assert list(out) == [-1] * 8
