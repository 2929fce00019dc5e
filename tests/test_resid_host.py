"""The residual layer on the CPU: tests/resid_reference.py (the format restated from its description) round-trips itself;
the host build of csrc/resid.inc -- through tests/resid_host_shim.cpp, compiled by g++ into a temporary directory --
equals it row by row and body by body; lbdrn_resid_info refuses damaged tables; the quantiser's properties hold over every
possible error; the container's trailer packs and unpacks; and tests/resid_damage_main.cpp, a stand-alone program built
with AddressSanitizer and UndefinedBehaviorSanitizer, feeds the host decoder damaged bodies.  No GPU.  Every comparison is
exact."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resid_reference as R  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
_vp, _i, _i64, _sz, _u32, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
_shim = None


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler (g++): the layer's host text cannot be compiled")
    return cxx


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        out = os.path.join(str(tmp_path_factory.mktemp("resid_shim")), "libresid_host_shim.so")
        subprocess.check_call([_cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                               os.path.join(ROOT, "tests", "resid_host_shim.cpp")])
        L = ctypes.CDLL(out)
        L.resid_shim_encode_row.argtypes = [_vp, _i, _vp, _i, _vp, _vp]
        L.resid_shim_decode_row.argtypes = [_vp, _u32, _u64, _u32, _i, _vp]
        L.resid_shim_quantise.argtypes = [_vp, _vp, _i64, ctypes.c_int32, _vp, _vp, _vp, _vp]
        L.resid_shim_max_symbol.argtypes = [ctypes.c_int32]
        L.resid_shim_max_symbol.restype = _u32
        L.resid_shim_bound.argtypes = [ctypes.c_int32] * 3
        L.resid_shim_bound.restype = _i64
        L.resid_shim_encode_body.argtypes = [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _i64]
        L.resid_shim_encode_body.restype = _i64
        L.resid_shim_info.argtypes = [_vp, _sz, _vp, _vp, _sz]
        L.resid_shim_decode_body.argtypes = [_vp, _sz] + [ctypes.c_int32] * 7 + [_vp]
        _shim = L
    return _shim


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


def _p(a):
    return a.ctypes.data_as(_vp)


def bits_of(data, n):
    return format(int.from_bytes(bytes(data), "big"), f"0{8 * len(data)}b")[:n] if n else ""


def shim_encode_row(L, us):
    u = np.ascontiguousarray(us, np.uint32)
    out = np.full(1400, 0x5A, np.uint8)
    k, costs = ctypes.c_int32(), np.zeros(16, np.uint32)
    n = L.resid_shim_encode_row(_p(u), u.size, _p(out), 1320, ctypes.byref(k), _p(costs))
    assert n >= 0, n
    assert (out[(n + 7) // 8:] == 0x5A).all()
    return bits_of(out[:(n + 7) // 8], n), k.value, costs


def shim_decode_row(L, bits, n, lead=0):
    """the row's bits placed `lead` bits into a buffer of exactly the bytes they need"""
    s = "1" * lead + bits
    s += "0" * (-len(s) % 8)
    data = np.frombuffer(int(s, 2).to_bytes(len(s) // 8, "big") if s else b"", np.uint8).copy() if s else np.zeros(0, np.uint8)
    buf = np.concatenate([data, np.full(64, 0xFF, np.uint8)])        # what lies behind must not be read as the row
    u = np.full(n + 8, 0xDEADBEEF, np.uint32)
    ok = L.resid_shim_decode_row(_p(buf), data.size, lead, len(bits), n, _p(u))
    assert (u[n:] == 0xDEADBEEF).all()
    return ok, u[:n]


def random_planes(rng, C, H, W, kind="mixed"):
    recon = rng.integers(0, 65536, (C, H, W)).astype(np.uint16)
    e = rng.integers(-6, 7, (C, H, W))
    if kind == "mixed":
        wide = rng.random((C, H, W)) < 0.03
        e = np.where(wide, rng.integers(-65535, 65536, (C, H, W)), e)
        e[:, : max(1, H // 5)] = np.where(rng.random((C, max(1, H // 5), W)) < 0.5, 0, e[:, : max(1, H // 5)]) * (rng.random((C, max(1, H // 5), 1)) < 0.5)
        e[:, :, W // 2:] *= rng.integers(1, 400, (C, H, 1))
    orig = np.clip(recon.astype(np.int64) + e, 0, 65535).astype(np.uint16)
    return orig, recon


GEOMETRIES = [(1, 1, 1), (1, 1, 300), (1, 300, 1), (2, 63, 255), (1, 64, 256), (3, 65, 257), (2, 130, 515)]


# ---------------------------------------------------------------- the reference alone

def test_reference_round_trips_itself():
    rng = np.random.default_rng(1)
    for (C, H, W), tau in zip(GEOMETRIES, (0, 1, 3, 0, 2, 7, 1)):
        orig, recon = random_planes(rng, C, H, W)
        body, want = R.encode_body(orig, recon, tau)
        assert int(np.abs(want.astype(np.int64) - orig).max()) <= tau
        assert np.array_equal(R.decode_body(body, recon), want)
        t, c, h, w, ext = R.parse_tables(body)
        assert (t, c, h, w) == (tau, C, H, W) and len(ext) == C * -(-H // 64) * -(-W // 256)
    # a rectangle reads only the blocks it touches
    orig, recon = random_planes(rng, 2, 130, 515)
    body, want = R.encode_body(orig, recon, 1)
    x0, y0, w, h = 250, 60, 20, 8
    got = R.decode_body(body, recon[:, y0:y0 + h, x0:x0 + w], (x0, y0, w, h))
    assert np.array_equal(got, want[:, y0:y0 + h, x0:x0 + w])


def test_reference_row_layout_by_hand():
    assert R.encode_row([0, 0, 0]) == ""
    assert R.encode_row([1]) == "0000" + "10"                        # k = 0: one one-bit, the zero
    assert R.encode_row([5, 4]) == "0001" + "110" + "1" + "110" + "0"   # k = 1 and k = 2 both take 8 bits (k = 0: 11): the lower
    assert R.encode_row([131071]) == "1111" + "1110" + "1" * 15             # k = 15: quotient 3, 19 bits; the escape would take 41
    assert R.encode_row([24] + [0] * 40) == "0000" + "1" * 24 + format(24, "017b") + "0" * 40     # k = 0: 41 + 40 (k = 1: 14 + 80)
    with pytest.raises(R.Damaged):
        R.decode_row("0000" + "10" + "0", 1)
    with pytest.raises(R.Damaged):
        R.decode_row("0000" + "1", 1)


# ---------------------------------------------------------------- the product's row coder against it

def test_row_fuzz_against_reference(shim):
    rng = np.random.default_rng(7)
    seen_k, ties, empty = np.zeros(16, int), 0, 0
    esc = {"q23": 0, "q24": 0, "q25": 0, "umax": 0}      # quotients under the row's chosen k: 23 is the last unary one, 24 and
                                                         # 25 are escaped; umax: u = 131071 with a quotient >= 24
    rows = []
    for n in (1, 2, 255, 256):
        rows.append(np.zeros(n, np.int64))
        for k in range(16):                     # magnitudes around 2^k make k (or a neighbour) the optimum
            rows.append(rng.integers(0, (3 << k) + 1, n))
            rows.append(rng.geometric(1.0 / (1 << k), n) - 1 if k else rng.integers(0, 2, n))
        for k in (0, 3, 9, 12):                 # the escape's edges under the parameter the row ends up with
            for q in (23, 24, 25):
                r = rng.integers(0, (3 << k) + 1, n)
                at, kk = int(rng.integers(0, n)), R.pick_k(r)
                for _ in range(4):              # (the outlier may move the optimum: follow it)
                    r[at] = min((q << kk) | int(rng.integers(0, 1 << kk)), 131071)
                    if R.pick_k(r) == kk:
                        break
                    kk = R.pick_k(r)
                rows.append(r)
        r = rng.integers(0, 131072, n)
        r[0] = 131071
        rows.append(r)
        rows.append(np.full(n, 131071))
    # u = 131071 ESCAPED: 41 one-bits, the only symbol whose unary run fills the reader's 32-bit look-ahead, and the whole
    # 17-bit raw field.  Alone or among large values a row takes k = 15 (quotient 3), so it needs company that keeps k <= 12.
    for n in (64, 255, 256):
        for small in (1, 4, 1 << 6, 1 << 12):
            r = rng.integers(0, small, n)
            r[rng.choice(n, 3, replace=False)] = 131071
            r[-1] = 131071                     # (also as the row's last symbol: nothing behind it to look ahead into)
            rows.append(r)
    rows += [np.array([2, 0]), np.array([1, 1, 3, 3]), np.array([4, 0, 4, 0])]     # ties between neighbours
    for _ in range(150):
        n = int(rng.choice([1, 2, 3, 17, 64, 255, 256]))
        rows.append(np.minimum(rng.integers(0, 1 << int(rng.integers(0, 18)), n) * (rng.random(n) < rng.random()), 131071))
    for us in rows:
        us = np.asarray(us, np.int64)
        want = R.encode_row(us)
        got, k, costs = shim_encode_row(shim, us)
        assert got == want, (us[:8], len(got), len(want))
        assert list(costs) == R.row_costs(us)
        if want == "":
            empty += 1
        else:
            assert k == R.pick_k(us) == int(want[:4], 2)
            seen_k[k] += 1
            c = R.row_costs(us)
            if c.count(min(c)) > 1:
                ties += 1
                assert k == c.index(min(c))
            for u in us:
                q = int(u) >> k
                esc["q23"] += q == 23
                esc["q24"] += q == 24
                esc["q25"] += q == 25
                esc["umax"] += int(u) == 131071 and q >= 24      # (counted only where it IS escaped)
        for lead in (0, 3, 13):
            ok, back = shim_decode_row(shim, want, us.size, lead)
            assert ok == 1 and np.array_equal(back, us), (lead, us[:8])
        assert R.decode_row(want, us.size) == [int(u) for u in us]
    assert (seen_k > 0).all(), f"parameters never chosen: {np.flatnonzero(seen_k == 0)}"
    assert ties > 0 and empty >= 4
    assert all(v > 0 for v in esc.values()), esc
    assert esc["umax"] >= 12, esc


def test_damaged_rows_are_refused_like_the_reference(shim):
    rng = np.random.default_rng(11)
    for _ in range(300):
        n = int(rng.choice([1, 2, 9, 64, 256]))
        us = rng.integers(0, 1 << int(rng.integers(1, 18)), n)
        bits = R.encode_row(us)
        if not bits:
            continue
        cut = int(rng.integers(1, len(bits)))
        for damaged in (bits[:cut], bits + "0" * int(rng.integers(1, 9)), bits[:cut] + ("1" if bits[cut] == "0" else "0") + bits[cut + 1:]):
            try:
                want = R.decode_row(damaged, n)
            except R.Damaged:
                want = None
            ok, back = shim_decode_row(shim, damaged, n, int(rng.integers(0, 8)))
            assert (ok == 1) == (want is not None)
            if want is not None:
                assert list(back) == want


# ---------------------------------------------------------------- whole bodies, info

def _shim_body(L, orig, recon, tau):
    C, H, W = orig.shape
    cap = L.resid_shim_bound(C, H, W)
    out = np.zeros(cap, np.uint8)
    n = L.resid_shim_encode_body(_p(np.ascontiguousarray(orig)), _p(np.ascontiguousarray(recon)), C, H, W, tau, _p(out), cap)
    assert n > 0
    return out[:n].tobytes()


def test_host_bodies_equal_the_reference(shim):
    rng = np.random.default_rng(3)
    for C, H, W in GEOMETRIES:
        orig, recon = random_planes(rng, C, H, W)
        for tau in (0, 1, 3):
            want_body, want = R.encode_body(orig, recon, tau)
            body = _shim_body(shim, orig, recon, tau)
            assert body == want_body, (C, H, W, tau)
            assert len(body) <= shim.resid_shim_bound(C, H, W)
            rec = recon.copy()
            assert shim.resid_shim_decode_body(body, len(body), C, H, W, 0, 0, W, H, _p(rec)) == 0
            assert np.array_equal(rec, want)
            out = np.zeros(4, np.int64)
            assert shim.resid_shim_info(body, len(body), _p(out), None, 0) == 0 and list(out) == [C, H, W, tau]
    # the bound counts 41 bits a sample; a row of extremes alone takes k = 15 (19 bits a sample): the escape needs a mixed row
    orig, recon = np.full((1, 65, 257), 65535, np.uint16), np.zeros((1, 65, 257), np.uint16)
    body = _shim_body(shim, orig, recon, 0)
    assert body == R.encode_body(orig, recon, 0)[0] and len(body) == 20 + 4 * 4 + sum(
        2 * rows + (rows * (4 + 19 * cols) + 7) // 8 for rows in (64, 1) for cols in (256, 1))


def _info():
    from lbdrn_hip import resid
    if not resid.available():
        pytest.fail("liblbdrn_resid.so is not built (python lbdrn-msic_amd/csrc/build.py)")
    return resid


def test_info_refuses_truncations_and_survives_corruptions():
    resid = _info()
    rng = np.random.default_rng(5)
    orig, recon = random_planes(rng, 2, 130, 515)
    body, _ = R.encode_body(orig, recon, 1)
    assert resid.info(body) == (2, 130, 515, 1)
    for n in sorted(set(int(v) for v in rng.integers(0, len(body), 200)) | {0, 19, 20, 20 + 4 * 18 - 1}):
        with pytest.raises(resid.ResidError):
            resid.info(body[:n])
    with pytest.raises(resid.ResidError):
        resid.info(body + b"\0")
    table_end = 20 + 4 * 18
    errors = 0
    for t in range(500):
        bad = bytearray(body)
        where = int(rng.integers(0, table_end)) if t % 2 else table_end + int(rng.integers(0, 2 * 64))      # tables of either kind
        bad[where] ^= 1 << int(rng.integers(0, 8))
        if t % 7 == 0:
            bad[int(rng.integers(0, table_end))] = int(rng.integers(0, 256))
        try:
            got = resid.info(bytes(bad))
        except resid.ResidError:
            errors += 1      # (refused: the product also refuses row lengths of 1..4 bits and lengths beyond the bound)
        else:       # a valid table: the reference agrees
            tau, C, H, W, ext = R.parse_tables(bytes(bad))
            assert got == (C, H, W, tau)
            for (c, y0, x0, rows, cols), (off, n) in zip(R.blocks_of(C, H, W), ext):
                R.decode_block(bytes(bad)[off:off + n], rows, cols, which=set())      # its row lengths add up
    assert errors > 100


# ---------------------------------------------------------------- quantiser

@pytest.mark.parametrize("tau", [0, 1, 2, 7, 65535])
def test_quantiser_properties_over_every_error(shim, tau):
    e = np.arange(-65535, 65536, dtype=np.int64)
    for name, orig, recon in (("orig = 0", np.zeros_like(e[e <= 0]), -e[e <= 0]),
                              ("orig = 65535", np.full_like(e[e >= 0], 65535), 65535 - e[e >= 0]),
                              ("recon low", np.maximum(e, 0), np.maximum(-e, 0)),
                              ("recon high", 65535 - np.maximum(-e, 0), 65535 - np.maximum(e, 0))):
        o32, r32 = orig.astype(np.int32), recon.astype(np.int32)
        q, u, back, rec = (np.zeros(o32.size, t) for t in (np.int32, np.uint32, np.int32, np.int32))
        shim.resid_shim_quantise(_p(o32), _p(r32), o32.size, tau, _p(q), _p(u), _p(back), _p(rec))
        assert np.array_equal(q, R.quantise(orig, recon, tau)), name
        assert np.array_equal(u, R.fold(q)) and np.array_equal(back, q) and np.array_equal(R.unfold(u), q), name
        assert int(u.max()) <= shim.resid_shim_max_symbol(tau) == R.max_symbol(tau) <= 131071
        assert np.array_equal(rec, R.enhance(recon, q, tau)), name
        assert int(np.abs(rec.astype(np.int64) - orig).max()) <= tau, name
        raw = R.enhance(recon, q, tau, clamp=False)
        assert int(np.abs(raw - orig).max()) <= tau
        over = (raw < 0) | (raw > 65535)
        if name.startswith("orig") and 0 < tau < 65535:      # (tau = 65535: q is 0 everywhere)  the clamp only ever moves recon' towards an in-range original
            assert np.array_equal(rec[over], orig[over])
            assert over.any() and int(np.abs(raw[over] - orig[over]).max()) == tau      # overshoot by exactly tau at the edge
        assert (np.abs(rec.astype(np.int64) - orig) <= np.abs(raw - orig)).all(), name
    # the fold is a bijection of the q range onto 0 .. max
    qs = np.arange(-(R.max_symbol(tau) // 2), R.max_symbol(tau) // 2 + 1)
    us = R.fold(qs)
    assert sorted(us.tolist()) == list(range(0, R.max_symbol(tau) + 1)) or tau == 65535
    assert np.array_equal(R.unfold(us), qs)


# ---------------------------------------------------------------- container

def test_trailer_packs_unpacks_and_leaves_the_header_alone():
    from lbdrn_hip import container
    nn, base = [b"n" * 11, b"N" * 7, b"n" * 5, b"n" * 3], [b"b" * 13, b"B" * 2, b"b" * 9, b"b" * 1]
    for act in ("sine", "relu"):
        header = container.pack_header(2, 300, 200, 5, 64, 2, 2, [len(x) for x in nn], [len(x) for x in base], activation=act)
        plain = header + b"".join(a + b for a, b in zip(nn, base))
        bodies = [b"LBR1" + bytes([k]) * (5 * k) for k in range(4)]
        trailer = container.pack_residual_trailer(3, bodies)
        assert trailer[:4] == b"LBRT" and trailer[4] == 1 and trailer[5:7] == b"\x00\x03"
        full = plain + trailer
        assert container.residual_trailer_offset(plain) == container.residual_trailer_offset(full) == len(plain)
        assert container.unpack_residual_trailer(plain) is None
        assert container.unpack_residual_trailer(full) == (3, bodies)
        assert container.unpack_header(full) == container.unpack_header(plain)
        assert container.header_activation(full) == container.header_activation(plain) == ("relu" if act == "relu" else None)
        for bad in (full[:-1], full + b"\0", plain + b"LBRX" + trailer[4:], plain + b"LBRT\x02" + trailer[5:], plain[:-1]):
            with pytest.raises(ValueError):
                container.unpack_residual_trailer(bad)
    with pytest.raises(OverflowError):
        container.pack_residual_trailer(65536, [])


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_damaged_bodies_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "resid_damage")
    cmd = [_cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), "-o", exe, os.path.join(ROOT, "tests", "resid_damage_main.cpp")]
    # does this compiler have the sanitizers' runtimes at all?  Asked of an empty program with the same flags, before the
    # program under test is touched: a failure of the real build below is then a failure, whatever its text.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "flagged" in run.stdout and "ERROR" not in run.stderr
