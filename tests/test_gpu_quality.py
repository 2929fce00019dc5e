"""Two rasters compared through liblbdrn_quality.so on the device (csrc/quality.hip): every field of the result against
tests/quality_reference.py on the shapes and data classes of tests/quality_helpers.py (the smallest at which the kernels can
go wrong: no window, one window, the SSIM tile's side - 1 / + 1, the statistics pass's row chunk - 1 / + 1, 16 bands, 8-bit
samples) and on one larger raster; a strided view against its contiguous copy; the C ABI on guarded buffers under three fills,
on two runs and on a second stream; the selection flags; and the command lines, decode.py --metrics and
python -m lbdrn_hip.quality.  Integer fields are compared exactly; the tolerances of the float64 fields are derived in
tests/quality_helpers.py.

Nothing here ran before the library existed: lbdrn_hip.quality and liblbdrn_quality.so are new."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_helpers as H  # noqa: E402
from guarded import FILLS, Arena  # noqa: E402

pytestmark = pytest.mark.gpu

_report = {}      # the largest distances from the reference seen in this run, printed by the last comparison test


def to_device(a, dev):
    import torch
    a = np.array(a, order="C")      # (a writable copy: torch wants one)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def device_compare(dev, a, b, peak, **kw):
    from lbdrn_hip import quality
    q = quality.compare(to_device(a, dev), to_device(b, dev), peak=peak, **kw)
    return q, H.unpack(q.raw, a.shape[0])


# ---------------------------------------------------------------- against the reference

@pytest.mark.parametrize("shape", H.SHAPES + (H.BIG_BAND_SHAPE,), ids=H.shape_id)
def test_device_equals_reference(dev, shape):
    import math
    cases = []
    if shape == H.BIG_BAND_SHAPE:
        cases.append(("big band", np.uint16, H.big_band()))
    else:
        for dtype in (np.uint16,) + ((np.uint8,) if shape in H.U8_SHAPES else ()):
            cases += [(name, dtype, ab) for name, ab in H.data_classes(shape, dtype).items()]
    for k, (name, dtype, (a, b)) in enumerate(cases):
        peak = H.peak_for(dtype, k)
        q, got = device_compare(dev, a, b, peak)
        want = H.reference((shape, name, np.dtype(dtype).name), a, b, peak)
        H.assert_matches(got, want, (shape, name, np.dtype(dtype).name), _report)
        if name == "identical":
            assert q.overall.sse == 0 and q.overall.psnr == math.inf and got["sam_sum"] == 0.0 and got["sam_max"] == 0.0
            assert all(r["ssim_sum"] == r["ssim_n"] and r["hist"][0] == r["n"] for r in got["bands"])      # SSIM exactly 1
        if name == "big band":
            assert got["bands"][0]["sse"] == 65 * 64 * 65535 ** 2 > 1 << 44
        if name == "zero pixels" and 2 <= shape[0] <= 16 and shape[1] * shape[2] > 16:
            assert got["sam_undefined"] > 0
    print(f"\nlargest distances so far: {_report}")


def test_larger_raster_and_host_arrays(dev):
    from lbdrn_hip import quality
    shape = (2, 1024, 1536)
    rng = np.random.default_rng(77)
    a = rng.integers(0, 65536, shape).astype(np.uint16)
    b = ((a & ~np.uint16(31)) | rng.integers(0, 32, shape).astype(np.uint16)).astype(np.uint16)
    q, got = device_compare(dev, a, b, 10000.0)
    H.assert_matches(got, H.reference("larger", a, b, 10000.0), "2 x 1024 x 1536", _report)
    print(f"\nlargest distances, the larger raster included: {_report}")
    # numpy arrays are uploaded and give the same bits; [H,W] is one band
    assert np.array_equal(quality.compare(a, b).raw, q.raw)
    one = quality.compare(a[0], b[0], sam=False)
    assert len(one.bands) == 1 and one.bands[0].sse == q.bands[0].sse and one.bands[0].ssim_sum == q.bands[0].ssim_sum


@pytest.mark.parametrize("dtype", (np.uint16, np.uint8), ids=("u16", "u8"))
def test_strided_view_equals_its_contiguous_copy(dev, dtype):
    from lbdrn_hip import quality
    rng = np.random.default_rng(4)
    top = 255 if dtype == np.uint8 else 65535
    sa, sb = (to_device(rng.integers(0, top + 1, (3, 60, 90)).astype(dtype), dev) for _ in range(2))
    peak = H.peak_for(dtype)
    for y0, x0, h, w in ((5, 7, 40, 61), (0, 8, 60, 33), (17, 1, 13, 89)):      # rows that do and do not start on 16 bytes
        va, vb = sa[:, y0:y0 + h, x0:x0 + w], sb[:, y0:y0 + h, x0:x0 + w]
        assert not va.is_contiguous()
        view = quality.compare(va, vb, peak=peak)
        copy = quality.compare(va.contiguous(), vb.contiguous(), peak=peak)
        assert np.array_equal(view.raw, copy.raw), (y0, x0, h, w)
        # one strided, one contiguous
        assert np.array_equal(quality.compare(va, vb.contiguous(), peak=peak).raw, copy.raw)


# ---------------------------------------------------------------- the C ABI on guarded buffers

def guarded_compare(dev, a, b, fill, what=3, short_by=0, stream=None, peak=10000.0):
    """lbdrn_quality_compare on buffers of tests/guarded.py: (rc, result words, arena, (result, workspace))"""
    import torch
    from lbdrn_hip import quality
    L = quality.lib()
    C, Hh, W = a.shape
    nres, nws = L.lbdrn_quality_result_bytes(C), L.lbdrn_quality_workspace(C, Hh, W, what)
    ar = Arena(dev)
    pa, pb = ar.const(a, name="a"), ar.const(b, name="b")
    res = ar.buf(nres, fill, name="result")
    ws = ar.buf(nws - short_by, fill, name="workspace")
    rc = L.lbdrn_quality_compare(pa.ptr, W, Hh * W, pb.ptr, W, Hh * W, a.dtype.itemsize * 8, C, Hh, W, peak, what, res.ptr, ws.ptr,
                                 nws - short_by, None if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, (res.numpy(np.uint64) if rc == 0 else None), ar, (res, ws)


def test_workspace_hygiene_and_determinism(dev):
    """fills 0x00 / 0xFF / 0xA5 of result and workspace give the same bits; the guards and the rasters are intact; two runs and
    a run on another stream give the same bits; a workspace one byte short is refused before a launch"""
    import torch
    from lbdrn_hip import quality
    for shape, dtype in (((4, 65, 129), np.uint16), ((16, 33, 70), np.uint8), ((1, 10, 40), np.uint16)):
        a, b = H.data_classes(shape, dtype)["zero pixels"]
        peak = H.peak_for(dtype)
        want = None
        for fill in FILLS + (0xA5,):      # (0xA5 twice: two runs)
            rc, words, ar, _ = guarded_compare(dev, a, b, fill, peak=peak)
            assert rc == 0, (quality.lib().lbdrn_quality_last_error(), fill)
            ar.check()
            want = words if want is None else want
            assert np.array_equal(words, want), (shape, fill)
        H.assert_matches(H.unpack(want, shape[0]), H.reference((shape, "zero pixels", np.dtype(dtype).name), a, b, peak), shape)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            rc, words, ar, _ = guarded_compare(dev, a, b, 0xFF, stream=side, peak=peak)
        ar.check()
        assert rc == 0 and np.array_equal(words, want)
        if shape[1] >= 11:
            rc, _, ar, bufs = guarded_compare(dev, a, b, 0xA5, short_by=1, peak=peak)
            assert rc == quality.E_WORKSPACE and b"workspace" in quality.lib().lbdrn_quality_last_error()
            ar.check()
            for buf in bufs:      # nothing was launched: every buffer still holds its fill
                assert bool((buf.as_u8() == 0xA5).all()), buf.name


def test_flags_leave_the_unselected_fields_zero(dev):
    shape = (4, 65, 129)
    a, b = H.data_classes(shape)["low 5 bits redrawn"]
    both = device_compare(dev, a, b, 10000.0)[1]
    none = device_compare(dev, a, b, 10000.0, ssim=False, sam=False)[1]
    only_ssim = device_compare(dev, a, b, 10000.0, sam=False)[1]
    only_sam = device_compare(dev, a, b, 10000.0, ssim=False)[1]
    stats = ("n", "sse", "sae", "sum_err", "max_abs", "hist")
    for r in (none, only_ssim, only_sam):
        assert [[band[k] for k in stats] for band in r["bands"]] == [[band[k] for k in stats] for band in both["bands"]]
    for r in (none, only_sam):
        assert all(band["ssim_n"] == 0 and band["ssim_sum"] == 0.0 for band in r["bands"])
    for r in (none, only_ssim):
        assert (r["sam_n"], r["sam_undefined"], r["sam_sum"], r["sam_max"]) == (0, 0, 0.0, 0.0)
    assert only_ssim["bands"] == both["bands"]
    assert all(only_sam[k] == both[k] for k in ("sam_n", "sam_undefined", "sam_sum", "sam_max")) and both["sam_n"] == 65 * 129
    # 17 bands: statistics of every band (two band blocks), no angle
    a17, b17 = np.concatenate([a] * 5)[:17], np.concatenate([b] * 5)[:17]
    wide = device_compare(dev, a17, b17, 10000.0)[1]
    assert wide["sam_n"] == 0 and wide["sam_sum"] == 0.0
    assert [band["sse"] for band in wide["bands"]] == [both["bands"][c % 4]["sse"] for c in range(17)]
    assert [band["hist"] for band in wide["bands"]] == [both["bands"][c % 4]["hist"] for c in range(17)]
    assert [band["ssim_sum"] for band in wide["bands"]] == [both["bands"][c % 4]["ssim_sum"] for c in range(17)]


# ---------------------------------------------------------------- the command lines

def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f]


def _split(path):
    """(the records that exist without --metrics apart from the time, the quality records)"""
    recs = _records(path)
    return [r for r in recs if not r.startswith(("Quality", "Time elapsed"))], [r for r in recs if r.startswith("Quality")]


@pytest.fixture(scope="module")
def streams(tmp_path_factory, dev):
    """two small .bin files (the shapes of tests/test_gpu_tiff_write.py): one image, -sr 1; four tiles with a residual layer
    of maximum error 2, -sr 2"""
    import encode
    from lbdrn_hip.synth import synthetic_tile
    root = tmp_path_factory.mktemp("quality_cli")
    saved = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = {}
    try:
        for name, shape, flags in (("one", (8, 40, 52), ["-K", "5", "-D", "2", "-bc", "64", "-nl", "2", "-sr", "1"]),
                                   ("layered", (4, 50, 37), ["-D", "1", "-sr", "2", "--max-error", "2"])):
            img = synthetic_tile(3 + len(name), *shape)
            src = str(root / f"{name}.npy")
            np.save(src, img)
            assert encode.main(["-i", src, "-o", str(root / name), "-e", "1", "-bs", "512"] + flags) == 0
            (sub,) = [d for d in (root / name).iterdir() if d.is_dir()]
            out[name] = (img, src, sub, str(sub / f"{name}.bin"))
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return out


@pytest.mark.parametrize("name", ("one", "layered"))
def test_decode_metrics_adds_its_records_and_changes_no_other(dev, streams, name, tmp_path, monkeypatch):
    import decode
    import results_summary
    from lbdrn_hip import quality, raster_io
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    img, src, sub, bin_path = streams[name]
    log, wlog = str(sub / "decode.txt"), str(sub / "decode_window.txt")
    x0, y0, w, h = 5, 7, 30, 21
    wout = str(tmp_path / "w.tif")

    def run(extra, window):
        path = wlog if window else log
        if os.path.exists(path):
            os.remove(path)
        argv = ["-i", bin_path, "-org", src] + (["--window", str(x0), str(y0), str(w), str(h), "-o", wout] if window else []) + extra
        assert decode.main(argv) == 0
        return _split(path)
    # the reconstruction, for the expected records
    assert decode.main(["-i", bin_path]) == 0
    rec = raster_io.read_raster(str(sub / f"{name}_recon.tif"))
    os.remove(log)
    for window in (False, True):
        plain, none = run([], window)
        assert none == [] and [r.split(":")[0] for r in plain if r.startswith(("MSE", "PSNR", "Max error", "Total size"))] == \
            ["MSE", "PSNR"] + (["Max error"] if name == "layered" else []) + ([] if window else ["Total size"])
        js = str(tmp_path / f"q{int(window)}.json")
        with_flag, lines = run(["--metrics", "--metrics-json", js], window)
        assert with_flag == plain      # line for line, apart from the time
        o, r = (img[:, y0:y0 + h, x0:x0 + w], rec[:, y0:y0 + h, x0:x0 + w]) if window else (img, rec)
        want = quality.compare(np.ascontiguousarray(o), np.ascontiguousarray(r))
        assert lines == want.to_records() and len(lines) == img.shape[0] + 1
        # directly behind PSNR / Max error
        recs = [x for x in _records(wlog if window else log) if not x.startswith("Time elapsed")]
        at = recs.index(lines[0])
        assert recs[at - 1].startswith("Max error" if name == "layered" else "PSNR") and recs[at:at + len(lines)] == lines
        d = json.load(open(js))
        ref = H.R.compare(o, r)
        for c, band in enumerate(d["bands"]):
            assert all(band[k] == ref["bands"][c][k] for k in ("n", "sse", "sae", "sum_err", "max_abs", "hist", "ssim_n"))
        assert (d["overall"]["sam_n"], d["overall"]["sam_undefined"]) == (ref["sam_n"], ref["sam_undefined"])
        if name == "layered":
            assert d["overall"]["max_abs"] <= 2
        # another peak changes PSNR and SSIM of the new records only
        other, lines255 = run(["--metrics", "--metrics-peak", "65535"], window)
        assert other == plain and lines255 == quality.compare(np.ascontiguousarray(o), np.ascontiguousarray(r), peak=65535.0).to_records()
        if not window:      # a results row parsed from the directory is the row without the flag
            row = results_summary.extract_metrics(log)
            run([], False)
            assert results_summary.extract_metrics(log) == row and set(row) == {"MSE", "PSNR", "bpsp", "bits"}


def test_module_command_line_in_a_child_process(dev, tmp_path):
    from lbdrn_hip import quality, raster_io
    a, b = H.data_classes((3, 12, 75))["low 5 bits redrawn"]
    pa, pb, pc = (str(tmp_path / n) for n in ("a.tif", "b.npy", "c.npy"))
    raster_io.write_raster(pa, a)
    np.save(pb, b)
    np.save(pc, b[:, :, :70])
    env = dict(os.environ, PYTHONPATH=os.path.join(H.ROOT, "lbdrn-msic_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    js = str(tmp_path / "q.json")

    def child(*args):
        return subprocess.run([sys.executable, "-m", "lbdrn_hip.quality"] + list(args), capture_output=True, text=True, env=env, timeout=300)
    run = child(pa, pb, "--json", js)
    assert run.returncode == 0, run.stderr
    want = quality.compare(a, b)
    assert run.stdout.splitlines() == want.to_records()
    assert json.load(open(js)) == json.loads(want.to_json())
    run = child(pa, pb, "--window", "3", "1", "40", "11", "--peak", "65535")
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == quality.compare(a[:, 1:12, 3:43], b[:, 1:12, 3:43], peak=65535.0).to_records()
    run = child(pa, pc)
    assert run.returncode == 2 and "shape" in run.stderr and run.stdout == ""
