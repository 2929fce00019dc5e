"""encode.py --nodata V --nodata-fit valid on the host: the argument errors (before any device work), what sweep.py and
run.sh pass on, the job formation that splits where n_valid differs, the valid pixels of hand-made masks, the step count, the
new record, and the plumbing of encode.main / main_k_points with the device work replaced by stand-ins (as
tests/test_nodata_host.py does).  The device side: tests/test_gpu_nodata_fit.py."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
for p in (PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_cli_sharding_cpu import _records  # noqa: E402
from test_nodata_host import ARGS, IMG, SUB, _collared, _stub_mask, _stub_nodata_layer  # noqa: E402
from test_resid_sharding_cpu import _stub_layer  # noqa: E402
from test_sweep_in_flight_host import _T, _payloads  # noqa: E402


# ---------------------------------------------------------------- the interface

def test_the_flag_is_in_the_header_and_the_wrapper_sets_it():
    from lbdrn_hip import _lib, ops
    with open(os.path.join(ROOT, "include", "lbdrn_hip.h")) as f:
        text = f.read()
    assert re.search(r"^#define LBDRN_EVAL_VALID 0x4000$", text, re.M) and _lib.EVAL_VALID == 0x4000
    assert re.search(r"^#define LBDRN_ABI_VERSION 2$", text, re.M)
    others = (_lib.EVAL_BACKGROUND, _lib.EVAL_FAST, _lib.EVAL_X16, _lib.APPLY_DECODE, 1, 2)
    assert all(_lib.EVAL_VALID & o == 0 for o in others)
    assert inspect.signature(ops.eval_sse).parameters["nodata"].default is None
    from lbdrn_hip import codec
    for fn in (codec.fit_device, codec.fit_group, codec.fit_many, codec.fit_image, codec.fit_images):
        assert inspect.signature(fn).parameters["nodata"].default is None


def test_apply_instance_ignores_the_flag_and_a_bad_field_is_refused_before_the_device():
    from lbdrn_hip import _lib
    lib = _lib.lib()
    for (C, H, W, bc, nl) in ((4, 30, 41, 64, 2), (8, 48, 130, 32, 1), (4, 30, 41, 256, 2)):
        F = C * 25
        net = _lib.Net(F, bc, C, nl, 0)
        for word in (0, _lib.EVAL_FAST, _lib.EVAL_FAST | _lib.EVAL_X16, _lib.EVAL_BACKGROUND):
            got = []
            for reserved, flag in ((0, 0), (0, _lib.EVAL_VALID), (70000, _lib.EVAL_VALID), (-5, _lib.EVAL_VALID)):
                g = _lib.Geom(C, H, W, 5, 2, 300, 1, 1, 0, reserved, None, None)
                out = (ctypes.c_int32 * 8)(*([-1] * 8))
                assert lib.lbdrn_apply_instance(ctypes.byref(g), ctypes.byref(net), word | flag, out) == 0
                got.append(list(out))
            assert got[0] == got[1] == got[2] == got[3]      # it selects no instance, and its field is not looked at here
    # lbdrn_eval_sse: the field outside 0..65535 is LBDRN_E_ARG, ahead of the device check and of every launch (the pointers
    # are never followed: the call ends at the argument checks; a workspace of 0 bytes would end it even behind them)
    net = _lib.Net(100, 64, 4, 2, 0)
    fake = ctypes.c_void_p(4096)
    for bad in (65536, -1, 1 << 20):
        g = _lib.Geom(4, 30, 41, 5, 2, 300, 1, 1, 0, bad, None, None)
        rc = lib.lbdrn_eval_sse(ctypes.byref(g), ctypes.byref(net), fake, fake, fake, fake, fake, 0, _lib.EVAL_VALID, None)
        assert rc == -1 and b"reserved" in lib.lbdrn_last_error()


# ---------------------------------------------------------------- the valid pixels, the step count

def test_valid_pixels_of_hand_made_masks():
    from lbdrn_hip import sampler
    img = np.full((3, 4, 5), 7, np.uint16)
    img[:, 0, :] = 0            # a void row: pixels 0..4
    img[1, 1, 2] = 0            # nodata in one band only: pixel 7 stays valid
    img[:2, 2, 3] = 0           # in two of three bands: pixel 13 stays valid
    img[:, 3, 4] = 0            # the last pixel void
    for V, planes in ((0, img), (40000, np.where(img == 0, 40000, img).astype(np.uint16)), (65535, np.where(img == 0, 65535, img).astype(np.uint16))):
        for t in (torch.from_numpy(planes.view(np.int16)), torch.from_numpy(planes.astype(np.int32))):
            vp = sampler.valid_pixels(t, V)
            assert vp.idx.dtype == torch.int64 and vp.idx.tolist() == list(range(5, 19)) and vp.n == 14 and vp.n_pixels == 20
            assert int(vp.samples) == int((planes != V).sum()) == 3 * 14 - 3 and vp.value == V
    none = sampler.valid_pixels(torch.from_numpy(img.view(np.int16)), 9)        # V nowhere: every pixel, the permutation as it is
    perm = torch.randperm(20)
    assert none.n == 20 and none.idx.tolist() == list(range(20)) and none.gather(perm) is perm and int(none.samples) == 60
    some = sampler.valid_pixels(torch.from_numpy(img.view(np.int16)), 0)
    perm = torch.randperm(14)
    assert torch.equal(some.gather(perm), some.idx[perm])
    empty = sampler.valid_pixels(torch.zeros((3, 4, 5), dtype=torch.int16), 0)
    assert empty.n == 0 and empty.idx.numel() == 0 and int(empty.samples) == 0 and empty.steps_per_epoch(8) == 0
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            sampler.valid_pixels(torch.zeros((1, 2, 2), dtype=torch.int16), bad)
    assert sampler.as_valid_pixels(None, None) is None and sampler.as_valid_pixels(None, some) is some


def test_steps_per_epoch_is_the_ceiling():
    from lbdrn_hip import sampler
    for n, bs, want in ((0, 256, 0), (1, 256, 1), (255, 256, 1), (256, 256, 1), (257, 256, 2), (2981888, 8192, 364), (4194304, 8192, 512),
                        (1, 1, 1), (7, 1, 7)):
        assert sampler.steps_per_epoch(n, bs) == want == -(-n // bs)


def test_form_jobs_splits_where_n_valid_differs():
    from lbdrn_hip import codec
    a, b, c = _T(1, 4, 24, 26), _T(2, 4, 24, 26), _T(3, 4, 24, 25)
    images, draws, Ks = [a, a, b, b, b, c], ["d"] * 6, [3, 4, 3, 4, 5, 3]
    old = codec.form_jobs(images, draws, Ks, 2)                          # the four-argument call: shapes alone decide
    assert [j[0] for j in old] == [[0, 1], [2, 3], [4], [5]] and all(len(j) == 4 for j in old)
    assert codec.form_jobs(images, draws, Ks, 2, None) == old and codec.form_jobs(images, draws, Ks, 2, [None] * 6) == old
    assert codec.form_jobs(images, draws, Ks, 2, [600] * 6) == old      # one n_valid everywhere: as without
    # the K points of one raster share n_valid and still group; another n_valid splits like another shape
    jobs = codec.form_jobs(images, draws, Ks, 3, [500, 500, 500, 400, 400, 400])
    assert [j[0] for j in jobs] == [[0, 1, 2], [3, 4], [5]]
    assert [j[3] for j in jobs] == [[3, 4, 3], [4, 5], [3]] and all(j[1] == [images[i] for i in j[0]] for j in jobs)
    assert [j[0] for j in codec.form_jobs(images, draws, Ks, 2, [624, None, 624, 624, 0, 0])] == [[0], [1], [2, 3], [4], [5]]
    # per-fit entries: one value for all, one per image, a raster named several times formed once
    t = torch.from_numpy(_collared().view(np.int16))
    vps = codec.valid_pixels_per_fit([t, t, t], 0)
    assert vps[0] is vps[1] is vps[2] and vps[0].n == int((~(_collared() == 0).all(0)).sum())
    mixed = codec.valid_pixels_per_fit([t, t, t], [None, 0, vps[0]])
    assert mixed[0] is None and mixed[1].n == vps[0].n and mixed[2] is vps[0]
    assert codec.valid_pixels_per_fit([t, t], None) == [None, None]
    with pytest.raises(ValueError):
        codec.valid_pixels_per_fit([t, t], [0])


# ---------------------------------------------------------------- the command lines

def test_argument_errors_come_before_any_device_work(tmp_path, monkeypatch, capsys):
    import encode
    import sweep
    from lbdrn_hip import shard

    def never(*a, **k):
        raise AssertionError("device work was started")
    for name in ("train_tiles", "train_tiles_at", "nodata_mask", "nodata_layer", "report_and_pack"):
        monkeypatch.setattr(encode, name, never)
    monkeypatch.setattr(shard, "init_host_group", never)
    monkeypatch.setattr(encode.raster_io, "read_raster", never)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    npy = str(tmp_path / "scene.npy")
    np.save(npy, IMG)
    out = tmp_path / "out"
    for extra in (["--nodata-fit", "valid"], ["--nodata-fit", "void", "--nodata", "0"], ["--nodata-fit", "--nodata", "0"],
                  ["--nodata-fit", "valid", "--nodata", "70000"]):
        with pytest.raises(SystemExit):
            encode.main(["-i", npy, "-o", str(out)] + extra + ARGS)
        with pytest.raises(SystemExit):
            encode.main_k_points(["-i", npy, "-o", str(out)] + extra + ARGS, (3, 4))
        assert "--nodata" in capsys.readouterr().err and not out.exists()
    # `all` asks for today's fit: with or without --nodata it is no error; absent flags leave no attribute behind
    parser = encode.build_parser()
    a = parser.parse_args(["-i", npy, "--nodata-fit", "all"])
    assert encode.nodata_value(parser, a) is None and encode.nodata_fit_mode(parser, a) == "all" and encode.fit_nodata(a) is None
    a = parser.parse_args(["-i", npy, "--nodata", "9", "--nodata-fit", "all"])
    assert encode.nodata_value(parser, a) == 9 and encode.fit_nodata(a) is None
    a = parser.parse_args(["-i", npy, "--nodata", "9", "--nodata-fit", "valid"])
    assert encode.nodata_value(parser, a) == 9 and encode.nodata_fit_mode(parser, a) == "valid" and encode.fit_nodata(a) == 9
    a = parser.parse_args(["-i", npy, "--nodata", "9"])
    assert not hasattr(a, "nodata_fit") and encode.nodata_value(parser, a) == 9 and encode.fit_nodata(a) is None
    # sweep.py refuses the same before any point is started
    with pytest.raises(SystemExit):
        sweep.parse(["--images", npy, "--nodata-fit", "valid"])
    with pytest.raises(SystemExit):
        sweep.parse(["--images", npy, "--nodata", "0", "--nodata-fit", "some"])


def test_sweep_and_run_sh_pass_the_option_on(tmp_path):
    import sweep
    got = sweep.common_args(sweep.parse(["--images", "a.tif", "--nodata", "0", "--nodata-fit", "valid"]))
    assert got[got.index("--nodata") + 1] == "0" and got[got.index("--nodata-fit") + 1] == "valid"
    got = sweep.common_args(sweep.parse(["--images", "a.tif", "--nodata", "tag", "--nodata-fit", "all"]))
    assert got[got.index("--nodata-fit") + 1] == "all"
    assert "--nodata-fit" not in sweep.common_args(sweep.parse(["--images", "a.tif", "--nodata", "0"]))
    assert "--nodata-fit" not in sweep.common_args(sweep.parse(["--images", "a.tif"]))
    import encode
    a = encode.build_parser().parse_args(["-i", "a.tif", "-K", "3"] + sweep.common_args(sweep.parse(["--images", "a.tif", "--nodata", "0", "--nodata-fit", "valid"])))
    assert a.nodata == "0" and a.nodata_fit == "valid"
    # run.sh: `python` is a stand-in that prints its arguments
    fake = tmp_path / "python"
    fake.write_text('#!/bin/bash\nprintf "%s\\n" "$@"\n')
    fake.chmod(0o755)
    positional = ["0", "2", "64", "2", "0.001", "8192", "10", "1", "outputs"]
    env = {k: v for k, v in os.environ.items() if k not in ("NGPU", "K_IN_FLIGHT", "PER_GPU", "KEEP_TAGS", "NODATA", "NODATA_FIT")}
    env.update(PATH=f"{tmp_path}:{env['PATH']}", PER_GPU="1")
    run = lambda e: subprocess.run(["bash", os.path.join(PKG, "run.sh")] + positional, env=e, capture_output=True, text=True,
                                   check=True).stdout.split("\n")[:-1]
    plain = run(env)
    assert plain == [os.path.join(PKG, "sweep.py")] + positional
    assert run(dict(env, NODATA="0", NODATA_FIT="valid")) == plain + ["--nodata", "0", "--nodata-fit", "valid"]
    assert run(dict(env, NODATA="0")) == plain + ["--nodata", "0"]
    s = sweep.parse(run(dict(env, NODATA="tag", NODATA_FIT="valid"))[1:])
    assert s.nodata == "tag" and s.nodata_fit == "valid" and sweep.parse(plain[1:]).nodata_fit is None


# ---------------------------------------------------------------- encode.py with stand-ins

class _Fit:
    """what a stand-in fit hands back: the payloads, and what the fit functions were given as `nodata`"""

    def __init__(self, payloads, tile, nodata):
        self.payloads = payloads
        self.n_valid = None if nodata is None else int((~(np.asarray(tile) == nodata).all(0)).sum())


SEEN = []


def _stub_train_tiles(args, tiles, draws):
    import encode
    SEEN.append(("main", encode.fit_nodata(args)))
    return [_Fit(_payloads(img, args.K, dr), img, encode.fit_nodata(args)) for (_, img), dr in zip(tiles, draws)]


def _stub_train_tiles_at(args, arrays, Ks, draws):
    import encode
    SEEN.append(("k_points", encode.fit_nodata(args)))
    return [_Fit(_payloads(img, K, dr), img, encode.fit_nodata(args)) for img, K, dr in zip(arrays, Ks, draws)]


def _stub_report(args, res, base_ahead=None):
    import logger
    nn, base = res.payloads
    logger.log.info(f"nn: {len(nn)} bytes, bpsp=0.5")
    logger.log.info(f"MSB: {len(base)} bytes: bpsp=0.25")
    return nn, base


def _stand_ins(monkeypatch, encode):
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles)
    monkeypatch.setattr(encode, "train_tiles_at", _stub_train_tiles_at)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    monkeypatch.setattr(encode, "residual_layer", _stub_layer)
    monkeypatch.setattr(encode, "nodata_mask", _stub_mask)
    monkeypatch.setattr(encode, "nodata_layer", _stub_nodata_layer)
    monkeypatch.setattr(encode, "BASE_CODEC", "LBB2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBDRN_TILE_READS"):
        monkeypatch.delenv(k, raising=False)
    del SEEN[:]


def test_the_record_and_what_the_fits_are_given(tmp_path, monkeypatch):
    import encode
    from LBDRNdataset import tile_windows
    assert encode.nodata_fit_record(2981888, 4194304, 8192) == "Nodata fit: 2981888 of 4194304 pixels, 364 steps per epoch"
    assert encode.nodata_fit_record(0, 130, 64) == "Nodata fit: 0 of 130 pixels, 0 steps per epoch"
    assert encode.nodata_fit_record(1, 130, 64) == "Nodata fit: 1 of 130 pixels, 1 steps per epoch"
    _stand_ins(monkeypatch, encode)
    img = _collared()
    src = str(tmp_path / "scene.npy")
    np.save(src, img)
    run = lambda name, extra: (encode.main(["-i", src, "-o", str(tmp_path / name)] + ARGS + extra),
                               (tmp_path / name / SUB / "scene.bin").read_bytes(), _records(tmp_path / name / SUB / "encode.txt"))[1:]
    masked, recs_masked = run("masked", ["--nodata", "0"])
    same, recs_all = run("all", ["--nodata", "0", "--nodata-fit", "all"])
    valid, recs_valid = run("valid", ["--nodata", "0", "--nodata-fit", "valid"])
    layered, recs_layered = run("layered", ["--nodata", "0", "--nodata-fit", "valid", "--max-error", "2"])
    assert SEEN == [("main", None), ("main", None), ("main", 0), ("main", 0)]
    strip = lambda rs, name: [r.replace(str(tmp_path / name), "X") for r in rs if not r.startswith(("Time elapsed", "Namespace"))]
    # `all` is the run without the option: the file, and every record but the one that prints the arguments
    assert same == masked and strip(recs_all, "all") == strip(recs_masked, "masked")
    # `valid`: one more record per tile, behind the tile's payload records; no other record changes (the stand-in payloads do not
    # depend on the option, so neither does the file: the format is the same)
    want = []
    for _, _, x0, y0, w, h in tile_windows(40, 31, 3):
        t = img[:, y0:y0 + h, x0:x0 + w]
        n = int((~(t == 0).all(0)).sum())
        want.append(f"Nodata fit: {n} of {w * h} pixels, {-(-n // 64)} steps per epoch")
    assert len(want) == 9 and any(" 0 of " in r for r in want) and len(set(want)) > 3
    assert [r for r in recs_valid if r.startswith("Nodata fit")] == want
    assert [r for r in strip(recs_valid, "valid") if not r.startswith("Nodata fit")] == strip(recs_masked, "masked") and valid == masked
    for k, r in enumerate(recs_valid):
        if r.startswith("Nodata fit"):
            assert recs_valid[k - 1].startswith("MSB: ") and recs_valid[k + 1].startswith("Nodata: V=0")
    assert [r for r in recs_layered if r.startswith("Nodata fit")] == want
    assert not any(r.startswith("Nodata fit") for r in recs_masked + recs_all)
    import results_summary as RS
    for pattern in [p for p, _ in RS.DECODE_RECORDS.values()] + [RS.ELAPSED] + list(RS.ENCODE_RECORDS.values()):
        assert pattern.search(want[0]) is None
    # main_k_points: the same files and records as point after point
    Ks = (3, 4)
    sub = lambda K: SUB.replace("_K4_", f"_K{K}_")
    common = [a for a in ARGS if a not in ("-K", "4")]
    for K in Ks:
        assert encode.main(["-i", src, "-o", str(tmp_path / "one"), "-K", str(K), "--nodata", "0", "--nodata-fit", "valid"] + common, shard_tiles=False) == 0
    del SEEN[:]
    assert encode.main_k_points(["-i", src, "-o", str(tmp_path / "many"), "--nodata", "0", "--nodata-fit", "valid"] + common, Ks) == {K: None for K in Ks}
    assert SEEN == [("k_points", 0)]
    for K in Ks:
        assert (tmp_path / "one" / sub(K) / "scene.bin").read_bytes() == (tmp_path / "many" / sub(K) / "scene.bin").read_bytes()
        a, b = (strip(_records(tmp_path / d / sub(K) / "encode.txt"), d) for d in ("one", "many"))
        assert a == b and [r for r in a if r.startswith("Nodata fit")] == want
