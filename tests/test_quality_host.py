"""The quality report on the CPU: the host build of csrc/quality.inc (tests/quality_host_shim.cpp, g++: the per-sample,
per-window and per-pixel text the device runs) against tests/quality_reference.py on the shapes and data classes of
tests/quality_helpers.py; the reference itself against scipy's Gaussian filter and against a brute-force evaluation in Python
integers; the library's checks that come before any launch; its size functions; the record lines; the kernels' resource
usage; and tests/quality_main.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer.
No GPU.  Integer fields are compared exactly; the tolerances of the float64 fields are derived in tests/quality_helpers.py."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_helpers as H  # noqa: E402
from quality_helpers import CSRC, ROOT  # noqa: E402

R = H.R


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return H.load_shim(tmp_path_factory)


# ---------------------------------------------------------------- the reference against two other evaluations

def test_reference_ssim_equals_scipy_gaussian_filter_cropped():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    assert abs(R.weights().sum() - 1.0) < 1e-15 and R.weights().argmax() == 5
    for shape, peak in (((23, 31), 10000.0), ((11, 11), 65535.0), ((40, 12), 10000.0)):
        a = rng.integers(0, 65536, shape).astype(np.uint16)
        b = ((a & ~np.uint16(31)) | rng.integers(0, 32, shape).astype(np.uint16)).astype(np.uint16)
        fa, fb = a.astype(np.float64), b.astype(np.float64)

        def blur(x):      # truncate = 3.5 at sigma 1.5: a radius of 5, the same 11 taps
            return ndimage.gaussian_filter(x, sigma=1.5, truncate=3.5)[5:-5, 5:-5]
        c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
        ma, mb = blur(fa), blur(fb)
        va, vb, cov = blur(fa * fa) - ma * ma, blur(fb * fb) - mb * mb, blur(fa * fb) - ma * mb
        want = ((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
        got = R.ssim_map(a, b, peak)
        assert got.shape == want.shape == (shape[0] - 10, shape[1] - 10)
        assert np.abs(got - want).max() <= H.SSIM_TOL


def test_reference_equals_a_brute_force_evaluation_in_python_integers():
    C, Hh, W = 2, 12, 13
    rng = np.random.default_rng(8)
    a = rng.integers(0, 65536, (C, Hh, W)).astype(np.uint16)
    b = rng.integers(0, 65536, (C, Hh, W)).astype(np.uint16)
    a[:, 0, 0] = 0          # undefined
    b[:, 0, 1] = 0          # undefined
    a[:, 0, 2] = 0
    b[:, 0, 2] = 0          # both: theta = 0
    peak = 10000.0
    ref = R.compare(a, b, peak)
    A, B = a.tolist(), b.tolist()
    w = R.weights().tolist()
    for c in range(C):
        es = [A[c][y][x] - B[c][y][x] for y in range(Hh) for x in range(W)]
        hist = [0] * 257
        for e in es:
            hist[min(abs(e), 256)] += 1
        rec = ref["bands"][c]
        assert (rec["n"], rec["sse"], rec["sae"], rec["sum_err"], rec["max_abs"], rec["hist"]) == \
            (Hh * W, sum(e * e for e in es), sum(abs(e) for e in es), sum(es), max(abs(e) for e in es), hist)
        vals = []
        for oy in range(Hh - 10):
            for ox in range(W - 10):      # the window as one 2-D weighted sum, not separated
                def mom(f):
                    return math.fsum(w[i] * w[j] * f(A[c][oy + i][ox + j], B[c][oy + i][ox + j]) for i in range(11) for j in range(11))
                ma, mb = mom(lambda p, q: p), mom(lambda p, q: q)
                va, vb, cov = mom(lambda p, q: p * p) - ma * ma, mom(lambda p, q: q * q) - mb * mb, mom(lambda p, q: p * q) - ma * mb
                c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
                vals.append(((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2)))
        assert rec["ssim_n"] == len(vals) == 2 * 3
        assert abs(rec["ssim_sum"] / rec["ssim_n"] - math.fsum(vals) / len(vals)) <= H.SSIM_TOL
    thetas, undefined = [], 0
    for y in range(Hh):
        for x in range(W):
            pa, pb = [A[c][y][x] for c in range(C)], [B[c][y][x] for c in range(C)]
            if not any(pa) and not any(pb):
                thetas.append(0.0)
            elif not any(pa) or not any(pb):
                undefined += 1
            else:
                dot = sum(p * q for p, q in zip(pa, pb))
                cross = sum((pa[i] * pb[j] - pa[j] * pb[i]) ** 2 for i in range(C) for j in range(i + 1, C))      # exact
                thetas.append(math.atan2(math.sqrt(cross), dot))
    assert (ref["sam_n"], ref["sam_undefined"]) == (len(thetas), undefined) == (Hh * W - 2, 2)
    assert abs(ref["sam_sum"] - math.fsum(thetas)) <= H.SAM_MEAN_RTOL * math.fsum(thetas)
    assert abs(ref["sam_max"] - max(thetas)) <= H.SAM_MAX_RTOL * max(thetas)


# ---------------------------------------------------------------- the host build against the reference

@pytest.mark.parametrize("shape", H.SHAPES + (H.BIG_BAND_SHAPE,), ids=H.shape_id)
def test_host_build_equals_reference(shim, shape):
    cases = []
    if shape == H.BIG_BAND_SHAPE:
        cases.append(("big band", np.uint16, H.big_band()))
    else:
        for dtype in (np.uint16,) + ((np.uint8,) if shape in H.U8_SHAPES else ()):
            cases += [(name, dtype, ab) for name, ab in H.data_classes(shape, dtype).items()]
    for k, (name, dtype, (a, b)) in enumerate(cases):
        peak = H.peak_for(dtype, k)
        got = H.unpack(H.shim_compare(shim, a, b, peak), shape[0])
        want = H.reference((shape, name, np.dtype(dtype).name), a, b, peak)
        H.assert_matches(got, want, (shape, name, np.dtype(dtype).name))
        if name == "identical":
            assert all(r["sse"] == 0 and r["hist"][0] == r["n"] for r in got["bands"]) and got["sam_sum"] == 0.0
            assert all(r["ssim_sum"] == r["ssim_n"] for r in got["bands"])      # SSIM is exactly 1 on equal windows
        if name == "big band":
            assert got["bands"][0]["sse"] == 65 * 64 * 65535 ** 2 > 1 << 44


def test_host_build_takes_strides_and_flags(shim):
    rng = np.random.default_rng(2)
    scene_a = rng.integers(0, 65536, (3, 40, 50)).astype(np.uint16)
    scene_b = rng.integers(0, 65536, (3, 40, 50)).astype(np.uint16)
    y0, x0, h, w = 3, 5, 20, 31
    wa, wb = scene_a[:, y0:y0 + h, x0:x0 + w], scene_b[:, y0:y0 + h, x0:x0 + w]
    whole = H.shim_compare(shim, wa, wb)
    out = np.zeros_like(whole)
    off = (y0 * 50 + x0) * 2
    rc = shim.quality_shim_compare(scene_a.ctypes.data + off, 50, 40 * 50, scene_b.ctypes.data + off, 50, 40 * 50, 16, 3, h, w, 10000.0, 3,
                                   out.ctypes.data)
    assert rc == 0 and np.array_equal(out, whole)
    none = H.unpack(H.shim_compare(shim, wa, wb, what=0), 3)
    assert all(r["ssim_n"] == 0 and r["ssim_sum"] == 0.0 for r in none["bands"]) and none["sam_n"] == none["sam_undefined"] == 0
    only_ssim, only_sam = H.unpack(H.shim_compare(shim, wa, wb, what=1), 3), H.unpack(H.shim_compare(shim, wa, wb, what=2), 3)
    both = H.unpack(whole, 3)
    assert only_ssim["bands"] == both["bands"] and only_ssim["sam_n"] == 0 and only_ssim["sam_sum"] == 0.0
    assert only_sam["sam_sum"] == both["sam_sum"] and all(r["ssim_n"] == 0 for r in only_sam["bands"])
    wide = H.unpack(H.shim_compare(shim, np.repeat(wa, 6, axis=0)[:17], np.repeat(wb, 6, axis=0)[:17]), 17)
    assert wide["sam_n"] == 0 and wide["sam_undefined"] == 0      # 17 bands: no angle


# ---------------------------------------------------------------- the library's checks that come before any launch

def test_library_refuses_before_any_launch(shim):
    from lbdrn_hip import quality
    L = quality.lib()
    assert L.lbdrn_quality_abi_version() == 1
    assert shim.quality_shim_stat_rows() == H.STAT_ROWS and shim.quality_shim_ssim_tile() == H.SSIM_TILE
    for C in (0, 1, 8, 16, 17, 65535, 65536, -1):
        assert L.lbdrn_quality_result_bytes(C) == shim.quality_shim_result_bytes(C) == (2112 * C + 32 if 1 <= C <= 65535 else 0)
    for C, Hh, W in ((1, 1, 1), (1, 10, 40), (8, 48, 80), (4, 65, 129), (16, 33, 70), (17, 33, 70), (8, 6000, 6000), (1, 1 << 20, 2048),
                     (1, 1 << 20, 2049), (0, 5, 5), (1, 0, 5), (1, 5, 0), (1, (1 << 20) + 1, 1)):
        for what in (0, 1, 2, 3):
            got = L.lbdrn_quality_workspace(C, Hh, W, what)
            assert got == L.lbdrn_quality_workspace(C, Hh, W, what) == shim.quality_shim_workspace(C, Hh, W, what)      # of its arguments alone
            ok = C >= 1 and 1 <= Hh <= 1 << 20 and 1 <= W <= 1 << 20 and Hh * W <= 1 << 31
            want = 0
            if ok and what & 2 and 2 <= C <= 16:
                want += 8 * -(-Hh // H.STAT_ROWS)
            if ok and what & 1 and Hh >= 11 and W >= 11:
                want += 8 * C * -(-(Hh - 10) // H.SSIM_TILE) * -(-(W - 10) // H.SSIM_TILE)
            assert got == want, (C, Hh, W, what)
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before any device work
    C, Hh, W = 8, 48, 80
    nws = L.lbdrn_quality_workspace(C, Hh, W, 3)
    assert nws == 8 * (12 + 8 * 2 * 3)

    def call(a=fake, b=fake, a_row=W, b_row=W, bits=16, C=C, Hh=Hh, W=W, peak=10000.0, what=3, result=fake, ws=fake, ws_bytes=nws):
        return L.lbdrn_quality_compare(a, a_row, Hh * a_row, b, b_row, Hh * b_row, bits, C, Hh, W, peak, what, result, ws, ws_bytes, None)
    err = L.lbdrn_quality_last_error
    for kw in (dict(a=None), dict(b=None), dict(result=None)):
        assert call(**kw) == quality.E_ARG and b"null" in err()
    for bits in (0, 12, 32):
        assert call(bits=bits) == quality.E_ARG and b"8 or 16" in err()
    for kw in (dict(C=0), dict(Hh=0), dict(W=0), dict(C=-3)):
        assert call(**kw) == quality.E_ARG and b"out of range" in err()
    assert call(a_row=W - 1) == quality.E_ARG and b"row strides" in err()
    assert call(b_row=W - 1) == quality.E_ARG and b"row strides" in err()
    for peak in (0.0, -1.0, math.nan, math.inf):
        assert call(peak=peak) == quality.E_ARG and b"peak" in err()
    assert call(what=4) == quality.E_ARG and b"what" in err()
    assert call(result=ctypes.c_void_p(4100)) == quality.E_ARG and b"aligned" in err()
    assert call(ws_bytes=nws - 1) == quality.E_WORKSPACE and b"workspace" in err()
    assert call(ws_bytes=0) == quality.E_WORKSPACE
    assert call(ws=None) == quality.E_WORKSPACE
    assert call(bits=12, ws_bytes=0) == quality.E_ARG      # precedence: E_ARG first


def test_python_refuses_mismatches_before_any_device_work():
    from lbdrn_hip import quality
    a = np.zeros((2, 5, 6), np.uint16)
    for b, word in ((np.zeros((2, 5, 7), np.uint16), "shape"), (np.zeros((3, 5, 6), np.uint16), "shape"), (np.zeros((5, 6), np.uint16), "shape"),
                    (np.zeros((2, 5, 6), np.uint8), "sample type"), (np.zeros((2, 5, 6), np.float32), "float32"),
                    (np.zeros((2, 5, 6), np.int16), "int16"), (np.zeros((1, 2, 5, 6), np.uint16), "shape"), ([[1]], "list")):
        with pytest.raises(ValueError, match=word):
            quality.compare(a, b)
    with pytest.raises(ValueError, match="peak"):
        quality.compare(a, a, peak=0)
    with pytest.raises(ValueError, match="empty"):
        quality.compare(np.zeros((2, 0, 6), np.uint16), np.zeros((2, 0, 6), np.uint16))


# ---------------------------------------------------------------- records

def _quality(shim, a, b, peak=10000.0):
    from lbdrn_hip import quality
    return quality.Quality(H.shim_compare(shim, a, b, peak), a.shape[0], peak, shape=a.shape)


def test_record_lines_round_trip_through_json_and_match_no_scraped_pattern(shim):
    from lbdrn_hip import quality
    import results_summary
    shape = (3, 12, 75)
    for name, (a, b) in list(H.data_classes(shape).items()) + [("no window", H.data_classes((1, 10, 40))["low 5 bits redrawn"])]:
        q = _quality(shim, a, b)
        lines = q.to_records()
        C = a.shape[0]
        assert len(lines) == C + 1 and lines[-1].startswith("Quality: ") and all(ln.startswith(f"Quality band {c}: ") for c, ln in enumerate(lines[:-1]))
        for ln in lines:
            for pat, _ in results_summary.DECODE_RECORDS.values():
                assert pat.search(ln) is None, ln
            assert results_summary.ELAPSED.search(ln) is None
            assert all(p.search(ln) is None for p in results_summary.ENCODE_RECORDS.values())
        d = json.loads(q.to_json())
        assert d["shape"] == list(a.shape) and d["peak"] == 10000.0

        def same(x, y):
            x, y = float(x), float(y)
            return (math.isnan(x) and math.isnan(y)) or x == y
        for c, ln in enumerate(lines[:-1]):
            band, vals = quality.parse_record(ln)
            j = d["bands"][c]
            assert band == c and vals["max"] == j["max_abs"] == q.bands[c].max_abs
            for rec, key in (("mse", "mse"), ("psnr", "psnr"), ("mae", "mae"), ("bias", "bias"), ("exact", "exact_share"), ("ssim", "ssim")):
                assert same(vals[rec], j[key]) and same(vals[rec], getattr(q.bands[c], key)), (name, rec)
            want = R.band_stats(a[c], b[c])
            assert all(j[k] == want[k] for k in want)      # the raw integers, histogram included
            assert j["mse"] == want["sse"] / want["n"] and j["bias"] == want["sum_err"] / want["n"]
        band, vals = quality.parse_record(lines[-1])
        o = d["overall"]
        assert band is None and vals["max"] == o["max_abs"]
        assert same(vals["mse"], o["mse"]) and same(vals["psnr"], o["psnr"]) and same(vals["mae"], o["mae"]) and same(vals["ssim"], o["ssim"])
        assert same(vals["sam_deg"], math.degrees(float(o["sam_mean"]))) and same(vals["sam_max_deg"], math.degrees(float(o["sam_max"])))
        if name == "identical":
            assert q.overall.psnr == math.inf and "psnr=inf" in lines[-1] and q.overall.ssim == 1.0 and q.overall.sam_mean == 0.0
            assert all(b_.exact_share == 1.0 for b_ in q.bands)
        if name == "no window":
            assert math.isnan(q.bands[0].ssim) and math.isnan(q.overall.sam_mean) and "ssim=nan" in lines[0]
    # the default peak is the fixed peak of the PSNR record
    a, b = H.data_classes(shape)["low 5 bits redrawn"]
    q = _quality(shim, a, b)
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    assert quality.DEFAULT_PEAK == 10000.0 and abs(q.overall.psnr - 10 * np.log10(10000 ** 2 / mse)) < 1e-12


def test_decode_refuses_the_metric_flags_without_their_partner(capsys):
    import decode
    for argv, word in ((["-i", "x.bin", "--metrics"], "-org"), (["-i", "x.bin", "-org", "o.npy", "--metrics-peak", "255"], "--metrics"),
                       (["-i", "x.bin", "-org", "o.npy", "--metrics-json", "q.json"], "--metrics"),
                       (["-i", "x.bin", "-org", "o.npy", "--metrics", "--metrics-peak", "0"], "positive")):
        with pytest.raises(SystemExit) as e:
            decode.main(argv, shard_tiles=False)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---------------------------------------------------------------- the kernels' resources

def test_no_kernel_of_the_library_has_scratch_or_spilled_registers():
    from lbdrn_hip import quality
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    if not os.path.exists(os.path.join(KR.LLVM, "llvm-objdump")) or not os.path.exists(quality._PATH):
        pytest.skip("llvm-objdump or the library is missing")
    rows = [r for r in KR.kernel_resources(quality._PATH) if "k_quality_" in r["demangled"]]
    names = " ".join(r["demangled"] for r in rows)
    assert all(k in names for k in ("k_quality_stats", "k_quality_ssim", "k_quality_finish")) and len(rows) == 7
    for r in rows:
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["spill_sgpr"] == 0, r
        if "k_quality_ssim" in r["demangled"]:      # two workgroups of the SSIM pass fit the 160 KB of a CU
            assert 2 * r["lds"] <= 160 * 1024 and r["vgpr"] + r["agpr"] <= 256, r


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_the_host_build_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "quality_main")
    cmd = [H.cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "quality_main.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "99 comparisons, 0 failed" in run.stdout and "ERROR" not in run.stderr
