"""Tiles whose MSB plane is zero everywhere (msb_max == 0: every sample below 2^K -- a dark or nodata corner of a scene, or
low-range data at a large K).  The reference divides by MSB.max() and gets 0 / 0 there; the library normalises such a plane
by 1 (include/lbdrn_hip.h, at msb_max), and so does the oracle: the features are exact zeros, and everything downstream is
finite and defined.  tests/test_thin_rasters_host.py holds the oracle's side on the CPU.

  * features, decode, evaluation and the fast passes on every path and every network of tests/thin_cases.py equal the oracle
    (4 x 9 x 12 and the thin 2 x 1 x 7), sigmoid outputs and sums finite;
  * the first training step against float64 as in tests/test_gpu_thin_rasters.py -- with relative colours every feature is
    zero, so only the biases and the layers behind the first learn --, loss and moments finite;
  * a group of four fits of one image at K = 3 .. 6 whose values lie in 8 .. 15 (the MSB plane is 1 everywhere at K = 3 and
    zero at K = 4, 5, 6: only some of a group's fits are dark) is bit-identical, fit by fit, to the single calls;
  * encode.py / decode.py on a 4-band 7 x 5 scene under -sr 3 whose top-left 2 x 1 tile is dark: lossless with
    --max-error 0, MSBs kept and every logged MSE finite without; and the lossless run on the all-noise scene, where every
    tile is thin and none is dark (which tells a thin-raster failure from a dark-tile one)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import thin_cases as TC  # noqa: E402
from lbdrn_hip import _lib, ops  # noqa: E402
from thin_gpu import bits, check_features, check_networks, first_step_against_float64, no_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
MFMA = _lib.PATH_MFMA
LR = 1e-3


@pytest.mark.parametrize("relative", (True, False), ids=("rel", "abs"))
@pytest.mark.parametrize("shape", TC.DARK_SHAPES, ids=lambda s: "C%d-%dx%d-D%d" % s)
def test_apply_side_of_a_dark_tile_equals_the_oracle(dev, shape, relative):
    C, H, W, D = shape
    case = TC.Case(C, H, W, D, relative)
    img = TC.dark_image(C, H, W)
    msb, lab, mx, img_d, msb_d, geom = check_features(dev, case, img)
    assert mx == 0 and geom.c.msb_max == 0 and not msb.any()
    assert not ops.features(geom, msb_d).view(torch.int32).any()            # +0.0f, every one
    worst = check_networks(dev, case, msb, lab, mx, img_d, msb_d, geom)
    print(f"\n{case.id} (dark): worst |fast - canonical| / canonical per network: "
          + ", ".join("bc%d-nl%d-%s %.1e" % (k + (v,)) for k, v in worst.items()))


DARK_TRAIN_ROWS = (
    TC.TrainRow("dark-stream-nl2-9x12", "k_train_stream", 64, 2, "sine", 4, 2, 9, 12),
    TC.TrainRow("dark-split-LQ24-9x12", "k_train_split", 64, 2, "sine", 4, 2, 9, 12, alone=True),
    TC.TrainRow("dark-stream-nl1-relu-1x7", "k_train_stream", 64, 1, "relu", 2, 2, 1, 7),
    TC.TrainRow("dark-tile-nl3-1x7", "k_train_mfma", 64, 3, "sine", 2, 2, 1, 7),
    TC.TrainRow("dark-half-bc256-9x12", "k_train_half", 256, 2, "sine", 4, 2, 9, 12),
)


def _dark_inputs(row):
    _, p0, perm = TC.train_inputs(row)
    return TC.dark_image(row.C, row.H, row.W), p0, perm


@pytest.mark.parametrize("row", DARK_TRAIN_ROWS, ids=repr)
def test_first_step_on_a_dark_tile_against_float64(dev, row):
    img, p0, perm = _dark_inputs(row)
    x, _, b, loss64, g64 = TC.first_step_f64(row, img, p0, perm)
    assert not x.any() and np.isfinite(loss64) and np.isfinite(g64).all() and np.abs(g64).max() > 0
    assert TC.kink_free(row, p0, x[b])
    first_step_against_float64(dev, row, (img, p0, perm))


def test_group_of_fits_of_which_some_are_dark(dev):
    """lbdrn_train_epoch_group takes every fit's own msb_max: 1, 0, 0, 0 here."""
    C, H, W, D, bs = 4, 9, 12, 2, 64
    rng = np.random.default_rng(3456)
    img = rng.integers(8, 16, (C, H, W)).astype(np.uint16)
    case = TC.Case(C, H, W, D)
    net = ops.make_net(case.F, 64, C, 2, ops.ACT_SINE)
    assert ops.train_group_size(C, H, W, 5, D, case.cfg(), 64, 2) == 4
    img_d = ops.to_device_u16(img, dev)
    perm = torch.from_numpy(rng.permutation(H * W).astype(np.int64)).to(dev)
    steps = (H * W + bs - 1) // bs
    fits = []
    for K in (3, 4, 5, 6):
        msb_d, mx = ops.split_bits(img_d, K)
        assert mx == (1 if K == 3 else 0)
        geom = ops.FeatureGeometry(C, H, W, K, D, mx, case.cfg(), dev)
        p0 = TC.rand_params(np.random.default_rng(K), case.F, 64, C, 2)
        ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img_d, msb_d, MFMA)
        fits.append(dict(K=K, msb=msb_d, geom=geom, p0=p0, ws=ws))

    def state(f):
        p = torch.from_numpy(f["p0"].copy()).to(dev)
        return [p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(steps, dtype=torch.float32, device=dev)]

    single = []
    for f in fits:
        st = state(f)
        for e in range(2):
            ops.train_epoch(f["geom"], net, img_d, f["msb"], perm, bs, st[0], st[1], st[2], e * steps, LR, st[3], MFMA, f["ws"])
        single.append([t.cpu().numpy() for t in st])
    sts = [state(f) for f in fits]
    for e in range(2):
        ops.train_epoch_group([f["geom"] for f in fits], net, [img_d] * 4, [f["msb"] for f in fits], [perm] * 4, bs,
                              [s[0] for s in sts], [s[1] for s in sts], [s[2] for s in sts], e * steps, LR, [s[3] for s in sts], MFMA,
                              [f["ws"] for f in fits])
    for f, st, want in zip(fits, sts, single):
        for name, a, c in zip(("params", "exp_avg", "exp_avg_sq", "losses"), st, want):
            a = a.cpu().numpy()
            assert np.isfinite(a).all(), (f["K"], name)
            assert np.array_equal(bits(a), bits(c)), (f["K"], name)
        assert np.abs(want[0] - f["p0"]).max() > 0
    assert len({s[3].tobytes() for s in single}) == 4                       # (four different fits: K changes the labels)


# ---------------------------------------------------------------------------------------------------------------------
# the command-line tools

def _scene(dark):
    """4 bands, 7 columns x 5 rows of 16-bit noise; -sr 3 cuts it into tiles of 2x1, 2x1, 3x1, 2x1, 2x1, 3x1, 2x3, 2x3, 3x3
    (w x h), every one thinner than the D = 2 window.  dark: the top-left 2 x 1 tile holds values below 2^5."""
    img = TC.noise_image(4, 5, 7, seed=11)
    if dark:
        img[:, 0:1, 0:2] = TC.dark_image(4, 1, 2, seed=11)
    return img


def _roundtrip(tmp_path, name, img, flags):
    import decode
    import encode
    from lbdrn_hip import raster_io
    src = str(tmp_path / f"{name}.tif")
    raster_io.write_raster(src, img)
    out = tmp_path / ("o_" + name)
    with no_ranks():
        assert encode.main(["-i", src, "-o", str(out), "-sr", "3", "-e", "2", "-bs", "256"] + flags) == 0
        (sub,) = [d for d in out.iterdir() if d.is_dir()]
        assert decode.main(["-i", str(sub / f"{name}.bin")]) == 0
    rec = raster_io.read_raster(str(sub / f"{name}_recon.tif")).reshape(img.shape)
    with open(sub / "encode.txt") as f:
        mses = [float(v) for v in re.findall(r"MSE: ([^\s)]+)\)", f.read())]
    return rec, mses


@pytest.mark.parametrize("dark", (True, False), ids=("dark-corner", "noise-only"))
def test_cli_lossless_on_a_scene_of_thin_tiles(dev, tmp_path, dark):
    img = _scene(dark)
    assert (int(img[:, 0:1, 0:2].max()) < 32) == dark and int(img[:, 0:1, 2:4].max()) >= 32
    rec, mses = _roundtrip(tmp_path, "dark" if dark else "noise", img, ["--max-error", "0"])
    assert len(mses) == 9 * 2 and np.isfinite(mses).all(), mses
    assert np.array_equal(rec, img)


def test_cli_lossy_on_a_scene_with_a_dark_tile(dev, tmp_path):
    img = _scene(True)
    rec, mses = _roundtrip(tmp_path, "lossy", img, [])
    print(f"\nper-tile, per-epoch MSE: {mses}")
    assert len(mses) == 9 * 2 and np.isfinite(mses).all(), mses
    assert np.array_equal(rec >> 5, img >> 5)
