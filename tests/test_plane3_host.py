"""LBB3 on the CPU: tests/plane3_reference.py (the format restated from include/lbdrn_plane3.h) round-trips itself; the host
build of csrc/plane3.inc -- through tests/plane3_host_shim.cpp, compiled by g++ into a temporary directory -- writes the same
bytes and each reads the other's; for one band in units as high as the raster it writes LBB2's bytes, by oracle/plane_codec.c
(the lane coder, csrc/plane_lane.inc, is one text for both formats); the rate against LBB2 on a scene whose bands share their structure and on one whose bands
do not; lbdrn_plane3_info refuses damaged tables; the container dispatches on the tag; and tests/plane3_damage_main.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, feeds the host decoder damaged bodies.
No GPU.  Every comparison is exact."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import plane3_reference as R  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
_vp, _i32, _i64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
CASES = R.cases()


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler (g++): the format's host text cannot be compiled")
    return cxx


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("plane3_shim")), "libplane3_host_shim.so")
    subprocess.check_call([_cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                           os.path.join(ROOT, "tests", "plane3_host_shim.cpp")])
    L = ctypes.CDLL(out)
    L.plane3_shim_bound.argtypes = [_i32] * 4
    L.plane3_shim_bound.restype = _i64
    L.plane3_shim_encode.argtypes = [_vp] + [_i32] * 4 + [_vp, _i64]
    L.plane3_shim_encode.restype = _i64
    L.plane3_shim_info.argtypes = [ctypes.c_char_p, _sz, _vp, ctypes.c_char_p, _sz]
    L.plane3_shim_decode.argtypes = [ctypes.c_char_p, _sz] + [_i32] * 4 + [_vp]
    return L


def _p(a):
    return a.ctypes.data_as(_vp)


def shim_encode(L, x, S=R.WRITER_S):
    x = np.ascontiguousarray(x, np.uint16)
    C, H, W = x.shape
    cap = L.plane3_shim_bound(C, H, W, S)
    out = np.full(cap + 16, 0x5A, np.uint8)
    n = L.plane3_shim_encode(_p(x), C, H, W, S, _p(out), cap)
    assert 0 < n <= cap, n
    assert (out[n:] == 0x5A).all()
    return out[:n].tobytes()


def shim_decode(L, body, C, H, W, S=R.WRITER_S):
    out = np.zeros((C, H, W), np.uint16)
    return L.plane3_shim_decode(bytes(body), len(body), C, H, W, S, _p(out)), out


def lbb2_bytes(x):
    import oracle as O
    counts, words = O.plane_encode(np.ascontiguousarray(x, np.uint16))
    return 4 * (counts.size + words.size)


# ---------------------------------------------------------------- the restatement alone

def test_reference_layout_by_hand():
    # one pixel of value 5: header, one unit of C + 1 + 1 words; the head word from best = fold(5 - 0) = 10, count = 1
    body = R.encode(np.array([[[5]]], np.uint16))
    w = np.frombuffer(body, "<u4")
    assert body[:4] == b"LBP3" and list(w[1:5]) == [1, 1, 1, 256] and w[5] == 3 and w.size == 9
    k0, z0 = R.start_parameters(10, 1)
    assert (k0, z0) == (3, 0) and w[6] == 3 and w[7] == 0                 # k0 = 3: 1 << 4 >= 10;  mode 0 on a tie
    # A = 6 << 3 = 48, N = 4: no group (2 A >= N); k = 3 (4 << 4 >= 48): q = 1 -> "10" + "010", padded
    assert w[8] == int("10010" + "0" * 27, 2)
    assert np.array_equal(R.decode(body), [[[5]]])
    # identical bands: band 1 takes the first differential mode, its residuals are zero and cost a flag per 16 samples
    x = np.repeat((np.arange(64 * 64).reshape(1, 64, 64) * 37 % 1000).astype(np.uint16), 2, axis=0)
    w = np.frombuffer(R.encode(x), "<u4")
    assert w[5 + 1 + 2] >> 3 == 4 and w[5 + 1 + 1] == 2 << 12                # mode word: band 1 = 4; band 1's head: z0 = 2


def test_reference_round_trips_itself():
    for name, x in CASES:
        if x.size > 40000:      # (the decoder is a Python loop per sample)
            continue
        body = R.case_body(name, x)
        C, H, W, S, units = R.parse(body)
        assert (C, H, W, S) == x.shape + (256,) and len(units) == -(-W // 64) * -(-H // 256)
        assert np.array_equal(R.decode(body), x), name
    x = dict(CASES)["2x65x64"]
    assert np.array_equal(R.decode(R.encode(x, 64)), x)


# ---------------------------------------------------------------- the host build of the format text against it

@pytest.mark.parametrize("name,x", CASES, ids=[n for n, _ in CASES])
def test_host_build_writes_the_same_bytes_and_each_reads_the_other(shim, name, x):
    want = R.case_body(name, x)
    body = shim_encode(shim, x)
    assert body == want, (len(body), len(want))
    rc, back = shim_decode(shim, want, *x.shape)              # the shim reads the restatement's bytes
    assert rc == 0 and np.array_equal(back, x)
    if x.size <= 40000:
        assert np.array_equal(R.decode(body), x)              # the restatement reads the shim's
    out = np.zeros(4, np.int64)
    assert shim.plane3_shim_info(body, len(body), _p(out), None, 0) == 0 and tuple(out) == x.shape + (256,)


@pytest.mark.parametrize("S", [64, 128, 512])
def test_other_unit_heights(shim, S):
    for name in ("3x257x65", "2x65x64", "16 bands"):
        x = dict(CASES)[name]
        body = shim_encode(shim, x, S)
        assert body == R.case_body(name, x, S)
        rc, back = shim_decode(shim, body, *x.shape, S)
        assert rc == 0 and np.array_equal(back, x)
    x = dict(CASES)["2x65x64"]
    assert np.array_equal(R.decode(shim_encode(shim, x, S)), x)


# ---------------------------------------------------------------- one lane coder: where the two formats coincide

def _lbb2_cases():
    from test_gpu_plane_codec import _cases      # LBB2's own case list (the module needs no GPU to import)
    return list(_cases())


LBB2_CASES = _lbb2_cases()


def _lbb2_strips(x):
    """the oracle's LBB2 body of x: the counts of all strips and then the strips, band-major -> [(count, words)] per strip"""
    import oracle as O
    counts, words = O.plane_encode(np.ascontiguousarray(x, np.uint16))
    ends = np.cumsum(counts.astype(np.int64))
    assert ends[-1] == words.size
    return [(counts[i], words[ends[i] - counts[i]:ends[i]]) for i in range(counts.size)]


def _lbb2_body(strips):
    return np.array([n for n, _ in strips], "<u4").tobytes() + b"".join(w.astype("<u4").tobytes() for _, w in strips)


@pytest.mark.parametrize("name,x", LBB2_CASES, ids=[n for n, _ in LBB2_CASES])
def test_shared_text_writes_lbb2_bytes(shim, name, x):
    """One band in units as high as the raster (S >= H): a unit is LBB2's strip, its head word and its one mode word a pass are
    LBB2's, and the body behind LBB3's 5-word header is LBB2's body byte for byte -- by oracle/plane_codec.c, which shares no
    text with csrc/plane_lane.inc."""
    x = x[:1]
    _, H, W = x.shape
    S = 64 * -(-H // 64)
    want = _lbb2_body(_lbb2_strips(x))
    assert shim_encode(shim, x, S)[4 * R.HEADER_WORDS:] == want
    rc, back = shim_decode(shim, R.MAGIC + struct.pack("<4I", 1, H, W, S) + want, 1, H, W, S)
    assert rc == 0 and np.array_equal(back, x)


def test_each_band_alone_is_its_strips_of_the_lbb2_body(shim):
    name, x = LBB2_CASES[7]
    assert name == "noise 8 bit" and x.shape == (3, 64, 64)
    strips = _lbb2_strips(x)
    assert len(strips) == 3      # one strip a band, band-major
    for c in range(3):
        assert shim_encode(shim, x[c:c + 1], 64)[4 * R.HEADER_WORDS:] == _lbb2_body(strips[c:c + 1]), c


# ---------------------------------------------------------------- rate

def test_rate_where_the_bands_share_their_structure():
    """LBB3 <= 0.90 x LBB2 on the model scene: a cap that fails if the differential modes are never taken (a static-Rice
    estimate of the mechanism gives 0.61 for 8 bands and 0.73 for 4)."""
    from lbdrn_hip.synth import correlated_tile
    for C in (8, 4):
        x = correlated_tile(0, C, 256, 256) >> 5
        n3, n2 = len(R.encode(x)), lbb2_bytes(x)
        print(f"correlated_tile(0, {C}, 256, 256) >> 5: LBB3 {n3} bytes, LBB2 {n2} bytes, ratio {n3 / n2:.4f}")
        assert n3 <= 0.90 * n2, (C, n3, n2)


# measured with the restatement (profiles/plane3_rate.txt): LBB3 / LBB2 on synthetic_tile(0, 8, 256, 256) >> K is 0.9736, 0.9584
# and 0.9229 -- LBB3 is the smaller one even where no band helps another, because ten modes share a word where LBB2 spends a
# word a strip and pass, and that outweighs the extra mode bit.  Each figure rounded up to the next half per cent:
INDEPENDENT_BANDS_CAP = {3: 0.975, 5: 0.960, 7: 0.925}


@pytest.mark.parametrize("K", [3, 5, 7])
def test_rate_where_the_bands_are_independent(K):
    from lbdrn_hip.synth import synthetic_tile
    x = synthetic_tile(0, 8, 256, 256) >> K
    n3, n2 = len(R.encode(x)), lbb2_bytes(x)
    print(f"synthetic_tile(0, 8, 256, 256) >> {K}: LBB3 {n3} bytes, LBB2 {n2} bytes, ratio {n3 / n2:.4f}")
    assert n3 <= INDEPENDENT_BANDS_CAP[K] * n2, (K, n3, n2)


def test_correlated_tile_is_what_the_issue_defines():
    """restated here draw by draw: default_rng(2000 + i); one shared field of six sinusoids drawn as synthetic_tile draws a
    band's, scaled to [0, 6000]; a shared N(0, 200^2) float32 noise; per band g, o, and clip(rint(o + g shared + N(0, 12^2)))"""
    import math
    from lbdrn_hip.synth import correlated_tile, synthetic_tile
    i, C, H, W = 3, 3, 40, 50
    rng = np.random.default_rng(2000 + i)
    yy = (np.arange(H, dtype=np.float32) / H)[:, None]
    xx = (np.arange(W, dtype=np.float32) / W)[None, :]
    acc = np.zeros((H, W), np.float32)
    for _ in range(6):
        fy, fx = rng.uniform(0.5, 6.0, 2)
        ph = rng.uniform(0, 2 * math.pi)
        amp = rng.uniform(0.3, 1.0)
        acc += np.float32(amp) * np.sin(np.float32(2 * math.pi) * (np.float32(fy) * yy + np.float32(fx) * xx) + np.float32(ph))
    shared = (acc - float(acc.min())) / (float(acc.max()) - float(acc.min())) * 6000.0
    shared = shared + rng.normal(0.0, 200.0, (H, W)).astype(np.float32)
    want = np.empty((C, H, W), np.uint16)
    for c in range(C):
        g = rng.uniform(0.6, 1.4)
        o = rng.uniform(300.0, 1500.0)
        want[c] = np.clip(np.rint(np.float32(o) + np.float32(g) * shared + rng.normal(0.0, 12.0, (H, W)).astype(np.float32)), 0, 16383)
    got = correlated_tile(i, C, H, W)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(correlated_tile(i, 2, H, W), want[:2])               # fewer bands: the same first bands
    big = correlated_tile(0, 4, 128, 128).astype(np.float64)
    assert min(np.corrcoef(big[0].ravel(), big[c].ravel())[0, 1] for c in range(1, 4)) > 0.99
    s = synthetic_tile(0, 4, 128, 128).astype(np.float64)                      # (unchanged, and its bands stay independent)
    assert max(abs(np.corrcoef(s[0].ravel(), s[c].ravel())[0, 1]) for c in range(1, 4)) < 0.9


# ---------------------------------------------------------------- container

def test_check_base_codec_accepts_lbb3_and_the_rest_as_before():
    from lbdrn_hip import container
    for name in ("LBB3", "LBB2", "LBB1", "jp2", "JP2", "jpeg2000", "jp2openjpeg", "jp2-gpu", "JP2-GPU"):
        assert container.check_base_codec(name) == name
    for name in ("lbb3", "lbb2", "LBB4", "jp3", "", "gpu"):
        with pytest.raises(ValueError):
            container.check_base_codec(name)


def test_container_dispatches_on_the_tag(monkeypatch):
    from lbdrn_hip import container, ops, plane3
    calls = []

    class FakePlanes:
        def __init__(self, a):
            self.a, self.shape = a, a.shape

    monkeypatch.setattr(ops, "to_device_u16", lambda a, device: FakePlanes(np.asarray(a, np.uint16)))
    monkeypatch.setattr(ops, "from_device_u16", lambda t: t.a)
    monkeypatch.setattr(plane3, "encode", lambda planes: calls.append(("encode", planes.shape)) or R.encode(planes.a))
    monkeypatch.setattr(plane3, "decode", lambda body, C, H, W, device: calls.append(("decode", (C, H, W))) or FakePlanes(R.decode(body)))
    monkeypatch.setattr(ops, "plane_encode", lambda planes: pytest.fail("LBB2's coder called for LBB3"))
    for dtype, code in ((np.uint16, 2), (np.uint8, 1)):
        msb = (np.arange(3 * 5 * 7).reshape(3, 5, 7) * 3 % 200).astype(dtype)
        payload = container.encode_base(msb, codec="LBB3")
        assert payload[:15] == b"LBB3" + struct.pack(">BHII", code, 3, 5, 7) and payload[15:] == R.encode(msb)
        back = container.decode_base(payload)
        assert back.dtype == dtype and np.array_equal(back, msb)
        kept = container.decode_base(payload, keep_on_device=True)
        assert isinstance(kept, FakePlanes) and np.array_equal(kept.a, msb)
        dev = FakePlanes(msb.astype(np.uint16))
        assert container.encode_base(dev, codec="LBB3", as_uint8=dtype == np.uint8) == payload
    assert [c[0] for c in calls] == ["encode", "decode", "decode", "encode"] * 2
    with pytest.raises(ValueError, match="16"):
        container.encode_base(np.zeros((17, 2, 2), np.uint16), codec="LBB3")
    with pytest.raises(ValueError, match="16"):
        container.encode_base(FakePlanes(np.zeros((17, 2, 2), np.uint16)), codec="LBB3")


def test_encode_py_takes_the_name_from_the_environment(monkeypatch):
    import importlib
    monkeypatch.setenv("LBDRN_BASE_CODEC", "LBB3")
    import encode as enc
    enc = importlib.reload(enc)
    try:
        assert enc.BASE_CODEC == "LBB3"
    finally:
        monkeypatch.delenv("LBDRN_BASE_CODEC")
        importlib.reload(enc)
    assert enc.BASE_CODEC == "LBB2"


# ---------------------------------------------------------------- lbdrn_plane3_info

def _info():
    from lbdrn_hip import plane3
    if not plane3.available():
        pytest.fail("liblbdrn_plane3.so is not built (python lbdrn-msic_amd/csrc/build.py)")
    return plane3


def test_info_validates_header_and_table():
    plane3 = _info()
    name = "3x257x65"
    x = dict(CASES)[name]
    body = R.case_body(name, x, 64)                      # 5 rows of units x 2
    assert plane3.info(body) == (3, 257, 65, 64)
    assert plane3.info(R.case_body(name, x)) == (3, 257, 65, 256)
    w = np.frombuffer(body, "<u4").copy()
    nunits, table = 10, 5

    def refused(words, what):
        with pytest.raises(plane3.Plane3Error, match=what):
            plane3.info(np.asarray(words, "<u4").tobytes())
    bad = w.copy(); bad[table + 3] = 0x7FFFFFFF
    refused(bad, "overrun")                              # a table entry that overruns the body
    refused(w[:table + 4], "cannot hold the table")      # a table of the wrong length: the body ends inside it
    refused(w[:table], "cannot hold the table")
    for S in (0, 1, 63, 65, 96, 100):
        bad = w.copy(); bad[4] = S
        refused(bad, "multiple of 64")                   # S
    bad = w.copy(); bad[4] = 128
    refused(bad, "add up|overrun|can take")              # another S: another table length, the counts no longer fit
    bad = w.copy(); bad[table] -= 1
    refused(bad, "add up")                               # counts that do not add up
    bad = w.copy(); bad[table] += 1
    refused(bad, "overrun|add up")
    refused(w[:-1], "overrun|add up")
    refused(np.concatenate([w, [0]]), "add up")
    bad = w.copy(); bad[table] -= 1; bad[table + 1] += 1
    assert plane3.info(bad.tobytes()) == (3, 257, 65, 64)       # (a word moved between units: the table is sound, the decoder flags it)
    bad = w.copy(); bad[0] ^= 1
    refused(bad, "not an LBB3 body")
    with pytest.raises(plane3.Plane3Error, match="not an LBB3 body"):
        plane3.info(body[:-1])                           # not a whole number of words
    for field, value in ((1, 0), (1, 17), (2, 0), (3, 0), (2, (1 << 20) + 1)):
        bad = w.copy(); bad[field] = value
        refused(bad, "out of range")
    bad = w.copy(); bad[table + nunits - 1] = 3          # fewer words than a unit's head, modes and first word
    refused(bad, "can take|add up")
    assert plane3.lib().lbdrn_plane3_bound(17, 4, 4) == 0 and plane3.lib().lbdrn_plane3_bound(16, 4, 4) > 0
    # the restatement agrees on every listed damaged body
    for dname, raw, geom in R.damaged_units():
        try:
            R.parse(raw)
            sound = True
        except R.Damaged:
            sound = False
        try:
            plane3.info(raw)
            ok = True
        except plane3.Plane3Error:
            ok = False
        assert ok == sound, dname


def test_bound_holds_and_matches_the_shim(shim):
    plane3 = _info()
    for C, H, W in ((1, 1, 1), (3, 257, 65), (16, 70, 66), (8, 2048, 2048), (4, 300, 333)):
        assert plane3.lib().lbdrn_plane3_bound(C, H, W) == shim.plane3_shim_bound(C, H, W, 256)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 65536, (2, 70, 70)).astype(np.uint16)          # noise: the costliest input there is
    assert len(shim_encode(shim, x)) <= plane3.lib().lbdrn_plane3_bound(2, 70, 70)


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_damaged_bodies_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "plane3_damage")
    cmd = [_cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), "-o", exe, os.path.join(ROOT, "tests", "plane3_damage_main.cpp")]
    # does this compiler have the sanitizers' runtimes at all?  Asked of an empty program with the same flags, before the
    # program under test is touched: a failure of the real build below is then a failure, whatever its text.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    listed = R.damaged_units()
    path = tmp_path / "damaged_units.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(listed)))
        for _, raw, geom in listed:
            f.write(struct.pack("<4iI", *geom, len(raw)) + raw)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"({len(listed)} listed)" in run.stdout and "flagged" in run.stdout and "ERROR" not in run.stderr
