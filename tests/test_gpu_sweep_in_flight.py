"""The K points of one image encoded side by side (encode.main_k_points, sweep.py --k-in-flight) write what the
point-after-point run writes: the same directories, byte-identical .bin files, the same encode.txt records apart from their
time fields, the same results CSV.

Input: a synthetic 4-band 16-bit TIFF of 51 x 47, so that -sr 2 gives four tiles of four shapes (26 / 25 columns x 24 / 23
rows); K = 3 .. 6, two epochs, minibatches of 256 rows."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
KS = (3, 4, 5, 6)
COMMON = ["-e", "2", "-bs", "256"]

# The time fields of an encode.txt record -- everything else of every record must agree:
#   "Time elapsed: <seconds>"                      the point's wall time
#   "<name>: fit <seconds>s on <device>"           wall time per tile with the others in flight
#   "... coded beside the fit; waited <seconds>s more for it"   (LBDRN_BASE_CODEC=jp2 only)
TIME_FIELDS = ((re.compile(r"^Time elapsed: .*$"), "Time elapsed: T"),
               (re.compile(r": fit [0-9.]+s on "), ": fit Ts on "),
               (re.compile(r"waited [0-9.]+s more"), "waited Ts more"))


def _records(path, root):
    out = []
    with open(path) as f:
        for line in f:
            rec = re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")).replace(str(root), "ROOT")
            for pat, to in TIME_FIELDS:
                rec = pat.sub(to, rec)
            out.append(rec)
    return out


def _folder(sr, K, max_error=None):
    return f"scene_r{sr}_K{K}_bc64_nl2_D2_prec16_lr0.001_bs256_e2"


@pytest.fixture(scope="module")
def scene(tmp_path_factory, dev):
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import synthetic_tile
    path = str(tmp_path_factory.mktemp("scene") / "scene.tif")
    raster_io.write_raster(path, synthetic_tile(11, 4, 47, 51))
    assert raster_io.read_raster(path).shape == (4, 47, 51)
    return path


@pytest.mark.parametrize("sr,base_codec,max_error", [(1, "LBB2", None), (2, "LBB2", None), (1, "jp2-gpu", None),
                                                     (2, "jp2-gpu", None), (2, "LBB2", 1)],
                         ids=["sr1", "sr2", "sr1-jp2gpu", "sr2-jp2gpu", "sr2-maxerror1"])
def test_bin_files_and_records_equal_the_point_after_point_run(dev, scene, tmp_path, monkeypatch, sr, base_codec, max_error):
    import encode
    monkeypatch.setattr(encode, "BASE_CODEC", base_codec)
    monkeypatch.setattr(encode, "DEVICE", "cuda:0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    extra = COMMON + ["-sr", str(sr)] + (["--max-error", str(max_error)] if max_error is not None else [])
    one, many = tmp_path / "one", tmp_path / "many"
    for K in KS:
        assert encode.main(["-i", scene, "-o", str(one), "-K", str(K)] + extra, shard_tiles=False) == 0
    outcome = encode.main_k_points(["-i", scene, "-o", str(many)] + extra, KS)
    assert outcome == {K: None for K in KS}
    bins = set()
    for K in KS:
        a, b = one / _folder(sr, K) / "scene.bin", many / _folder(sr, K) / "scene.bin"
        assert a.read_bytes() == b.read_bytes(), K
        bins.add(a.read_bytes())
        ra, rb = _records(one / _folder(sr, K) / "encode.txt", one), _records(many / _folder(sr, K) / "encode.txt", many)
        assert ra == rb, K
        assert sum(r.startswith("nn: ") for r in rb) == sr * sr and rb[-1] == "Time elapsed: T"
        assert sum(r.startswith("Residual layer: ") for r in rb) == (sr * sr if max_error is not None else 0)
        assert sorted(os.listdir(one / _folder(sr, K))) == sorted(os.listdir(many / _folder(sr, K)))
    assert len(bins) == len(KS)
    # a second call finds every point finished, like main()
    assert encode.main_k_points(["-i", scene, "-o", str(many)] + extra, KS) == {K: None for K in KS}


def test_sweep_cli_with_k_in_flight_equals_the_default(dev, scene, tmp_path, monkeypatch):
    import sweep
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    args = ["--images", scene, "--k", str(KS[0]), str(KS[-1]), "--summary"] + COMMON
    one, many = tmp_path / "one", tmp_path / "many"
    assert sweep.main(args + ["-o", str(one)]) == 0
    assert sweep.main(args + ["-o", str(many), "--k-in-flight", "4"]) == 0
    listing = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    assert listing(one) == listing(many)
    assert len([f for f in listing(one) if f.endswith(".bin")]) == len(KS)
    csvs = [f for f in listing(one) if f.endswith(".csv")]
    assert len(csvs) == 1
    for f in listing(one):
        if f.endswith((".bin", ".csv")):
            assert (one / f).read_bytes() == (many / f).read_bytes(), f
    rows = (one / csvs[0]).read_text().splitlines()
    assert len(rows) == 1 + len(KS) and all(cell for row in rows for cell in row.split(","))     # every point has its metrics
