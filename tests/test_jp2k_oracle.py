"""The JPEG 2000 oracle (oracle/jp2k_oracle.c through oracle/jp2k.py) proves itself on the CPU -- round trips, the transform
and the tier-1 decoder inverting, OpenJPEG and Pillow reading its files and it theirs, a committed fixture of files
OpenJPEG wrote -- and then judges the product's host-compilable text (csrc/jp2k_t1.inc, jp2k_t2.inc through
oracle/jp2k_host_shim.cpp) stage by stage: block coder, byte clamp, packet headers, geometry, whole files.  No GPU.
Every comparison is exact.  tests/test_gpu_jp2k.py imports the case lists below for the device."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import jp2k  # noqa: E402
from test_jp2k_host import GEOMETRIES  # noqa: E402

F = jp2k.F

# (H, W) beyond GEOMETRIES: sides of exactly 1024 and of 1025, one-pixel-wide last tiles, H = 1 with W > 1024 (tiled, one
# resolution), three or more tiles per axis with a ragged last tile, 32768 on one side
NEW_GEOMETRIES = [(1024, 300), (300, 1024), (1025, 300), (300, 1025), (1025, 1025), (1025, 2049), (64, 1025), (1, 1500), (1, 2049),
                  (3000, 2500), (2049, 3100), (3, 3073), (32768, 3), (2, 32768), (32768, 1)]
# the ones small enough to code whole planes of (the 32768-long ones as thin strips)
NEW_GEOMETRY_PLANES = [(1, 1024, 300), (2, 300, 1024), (1, 1025, 300), (1, 300, 1025), (1, 1025, 1025), (1, 1025, 2049), (3, 64, 1025),
                       (2, 1, 1500), (1, 1, 2049), (1, 3000, 2500), (1, 2049, 3100), (2, 3, 3073), (1, 32768, 3), (1, 2, 32768),
                       (1, 32768, 1)]
SMALL_SHAPES = [(1, 1, 1), (2, 1, 200), (1, 33, 70), (3, 300, 517), (5, 1025, 64), (1, 2, 2), (1, 3000, 1), (2, 65, 129), (1, 64, 64),
                (1, 5, 1030), (1, 1029, 1061)]
STATISTICS = ["synth", "zero", "mid", "constant", "spike", "uniform", "sparse", "stripes_h", "stripes_v", "checker", "low_bits"]


def planes_of(stat, shape, bits=16, seed=0):
    """[C, H, W] test planes of a named statistic"""
    C, H, W = shape
    top = (1 << bits) - 1
    rng = np.random.default_rng([seed, C, H, W, bits, STATISTICS.index(stat)])
    yy, xx = np.mgrid[0:H, 0:W]
    if stat == "synth":
        from lbdrn_hip.synth import synthetic_tile
        x = synthetic_tile(seed, C, H, W) >> (5 if bits == 16 else 8)
    elif stat == "zero":
        x = np.zeros(shape)
    elif stat == "mid":                      # zero after the level shift: no block has a pass
        x = np.full(shape, 1 << (bits - 1))
    elif stat == "constant":
        x = np.full(shape, 1234 % top)
    elif stat == "spike":
        x = np.zeros(shape)
        x[C - 1, int(rng.integers(H)), int(rng.integers(W))] = top
    elif stat == "uniform":
        x = rng.integers(0, top + 1, shape)
    elif stat == "sparse":
        x = np.where(rng.random(shape) < 0.01, rng.integers(0, top + 1, shape), 1 << (bits - 1))
    elif stat == "stripes_h":                # period-2 patterns of 0 / top: the largest high-pass magnitudes
        x = np.broadcast_to((yy & 1) * top, shape)
    elif stat == "stripes_v":
        x = np.broadcast_to((xx & 1) * top, shape)
    elif stat == "checker":
        x = np.broadcast_to(((xx ^ yy) & 1) * top, shape)
    elif stat == "low_bits":
        x = rng.integers(0, 4, shape) + (1 << (bits - 1)) - 2
    else:
        raise KeyError(stat)
    return np.ascontiguousarray(x).astype(np.uint16 if bits == 16 else np.uint8)


def fuzz_planes(n, seed, max_side=140):
    """n seeded random (C, H, W, bits, statistic) cases; every fifth one is tiled (one long side)"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        C = int(rng.integers(1, 4))
        H, W = (int(v) for v in rng.integers(1, max_side, 2))
        if k % 5 == 4:
            if rng.integers(2):
                H = int(rng.integers(1025, 1100))
            else:
                W = int(rng.integers(1025, 1100))
        bits = 8 if rng.integers(3) == 0 else 16
        stat = STATISTICS[int(rng.integers(len(STATISTICS)))]
        yield (C, H, W), bits, stat, planes_of(stat, (C, H, W), bits, seed=k)


def has_empty_packet(buf):
    """whether some packet of the file carries no block (however the writer spelled it)"""
    i, rec = jp2k.info(buf), jp2k.parse(buf)
    inc = rec[rec[:, F["passes"]] > 0]
    full = {(int(r[F["tile"]]), int(r[F["comp"]]), int(r[F["res"]])) for r in inc}
    return len(full) < i["tiles"] * i["C"] * i["resolutions"]


def openjpeg():
    from lbdrn_hip import jp2
    if not jp2.available():
        pytest.skip("liblbdrn_jp2.so not built (OpenJPEG absent): this leg needs OpenJPEG")
    return jp2


# ------------------------------------------------------------------ 1. the oracle proves itself

@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_decodes_what_it_encodes(shape):
    stats = STATISTICS if shape[1] * shape[2] < 400000 else ["synth", "uniform", "checker", "spike"]
    for stat in stats:
        for bits in (16, 8):
            x = planes_of(stat, shape, bits)
            f = jp2k.encode(x)
            y = jp2k.decode(f)
            assert y.dtype == x.dtype and np.array_equal(y, x), (shape, stat, bits)
            rec = jp2k.parse(f)
            assert len(rec) == jp2k.info(f)["blocks"] == len(jp2k.blocks(*shape, bits))
            assert (rec[:, F["numbps"]] <= rec[:, F["mb"]]).all(), (shape, stat, bits)


def test_oracle_round_trips_a_seeded_fuzz():
    for shape, bits, stat, x in fuzz_planes(40, 20261016):
        assert np.array_equal(jp2k.decode(jp2k.encode(x)), x), (shape, bits, stat)


def test_transform_inverts_exactly_and_is_the_53_filter():
    rng = np.random.default_rng(53)
    for h, w in [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (64, 64), (37, 53), (128, 100), (1, 2), (2, 1)]:
        for x0, y0 in [(0, 0), (1024, 2048), (3, 5), (1, 0)]:
            a = rng.integers(-40000, 40000, (h, w)).astype(np.int32)
            for levels in range(0, 6):
                f = jp2k.dwt53(a, levels, x0, y0)
                assert np.array_equal(jp2k.dwt53(f, levels, x0, y0, inverse=True), a), (h, w, x0, y0, levels)
    # one level on a line against the filter written out: d[n] = x[2n+1] - floor((x[2n] + x[2n+2]) / 2),
    # s[n] = x[2n] + floor((d[n-1] + d[n] + 2) / 4), whole-sample symmetric extension
    x = rng.integers(-1000, 1000, 11).astype(np.int64)
    e = lambda i: x[abs(i) if i < 11 else 20 - i]   # noqa: E731
    d = {n: e(2 * n + 1) - ((e(2 * n) + e(2 * n + 2)) >> 1) for n in range(-1, 6)}
    s = [e(2 * n) + ((d[n - 1] + d[n] + 2) >> 2) for n in range(6)]
    f = jp2k.dwt53(x[None].astype(np.int32), 1)
    assert f[0].tolist() == s + [d[n] for n in range(5)]
    # a constant plane has no high-pass energy
    f = jp2k.dwt53(np.full((20, 30), 7, np.int32), 3)
    assert (f[:3, :4] == 7).all() and f.sum() == 7 * 12


def test_fixture_of_openjpeg_files_decodes_parses_and_matches(golden):
    g = golden["jp2k_openjpeg"]
    names = sorted(k[len("file_"):] for k in g.files if k.startswith("file_"))
    assert len(names) >= 6
    seen_empty = seen_tiled = 0
    for name in names:
        x, f = g["planes_" + name], g["file_" + name].tobytes()
        y = jp2k.decode(f)
        assert y.dtype == x.dtype and np.array_equal(y, x), name
        i = jp2k.info(f)
        assert (i["C"], i["H"], i["W"]) == x.shape and i["bits"] == 8 * x.dtype.itemsize
        seen_tiled += i["tiles"] > 1
        mine = jp2k.encode(x)
        assert np.array_equal(jp2k.parse(mine)[:, [F["numbps"], F["passes"], F["length"]]],
                              jp2k.parse(f)[:, [F["numbps"], F["passes"], F["length"]]]), name
        if has_empty_packet(f):
            seen_empty += 1
        else:
            assert jp2k.tile_parts(mine) == jp2k.tile_parts(f), jp2k.first_difference(mine, f, x)
    assert seen_empty >= 1 and seen_tiled >= 2


def test_openjpeg_and_the_oracle_read_each_other_and_write_the_same_tile_parts():
    jp2 = openjpeg()
    compared = 0
    cases = [(s, 16, "synth") for s in SMALL_SHAPES] + [((3, 300, 517), 8, "synth"), ((2, 100, 130), 16, "uniform"),
                                                         ((2, 100, 130), 16, "checker"), ((1, 130, 140), 16, "spike"),
                                                         ((2, 100, 130), 16, "mid"), ((2, 90, 77), 8, "stripes_v")]
    cases += [(s, b, st) for s, b, st, _ in fuzz_planes(25, 7)]
    for shape, bits, stat in cases:
        x = planes_of(stat, shape, bits)
        mine, theirs = jp2k.encode(x), jp2.encode(x)
        assert np.array_equal(jp2.decode(mine), x), (shape, bits, stat)
        assert np.array_equal(jp2k.decode(theirs), x), (shape, bits, stat)
        if not has_empty_packet(theirs):
            assert jp2k.tile_parts(mine) == jp2k.tile_parts(theirs), (shape, bits, stat, jp2k.first_difference(mine, theirs, x))
            compared += 1
    assert compared >= 20


def test_pillow_and_the_oracle_read_each_other():
    from PIL import Image, features
    if not features.check_codec("jpg_2000"):
        pytest.skip("this Pillow has no JPEG 2000 codec")
    for shape, bits, stat in [((1, 300, 517), 16, "synth"), ((3, 300, 517), 8, "synth"), ((1, 33, 70), 8, "uniform"),
                              ((1, 90, 77), 16, "checker"), ((1, 1030, 70), 16, "synth")]:
        x = planes_of(stat, shape, bits)
        im = Image.open(io.BytesIO(jp2k.encode(x)))
        im.load()
        got = np.asarray(im)
        want = x[0] if shape[0] == 1 else x.transpose(1, 2, 0)
        assert np.array_equal(got.astype(x.dtype), want), (shape, bits, stat)
        buf = io.BytesIO()
        Image.fromarray(want).save(buf, "JPEG2000", irreversible=False, mct=0, num_resolutions=jp2k.layout(*shape, bits)[4])
        assert np.array_equal(jp2k.decode(buf.getvalue()), x), (shape, bits, stat)


# ------------------------------------------------------------------ 2. the product's host text against the oracle

@pytest.fixture(scope="module")
def shim():
    L = jp2k.shim()
    if L is None:
        pytest.skip("no host C++ compiler (g++): oracle/_build/libjp2k_host_shim.so is not built")
    return L


BLOCK_STATS = ["zero", "corner0", "corner1", "corner2", "corner3", "middle", "sparse", "dense", "constant_pos", "constant_neg",
               "alternating", "checker", "runlength"]
BIASED = [1, 2, 3, 4, 5, 63, 64]


def make_block(rng, w, h, numbps, stat):
    """[h, w] int32 coefficients whose largest magnitude has exactly `numbps` bits (all zero for "zero")"""
    top = (1 << numbps) - 1
    peak = int(rng.integers(1 << (numbps - 1), top + 1))
    sign = lambda shape: 1 - 2 * rng.integers(0, 2, shape)   # noqa: E731
    a = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    if stat == "zero":
        return a.astype(np.int32)
    if stat.startswith("corner"):
        k = int(stat[-1])
        a[(h - 1) * (k >> 1), (w - 1) * (k & 1)] = peak * int(sign(1)[0])
    elif stat == "middle":
        a[h // 2, w // 2] = peak * int(sign(1)[0])
    elif stat == "sparse":
        a = np.where(rng.random((h, w)) < 0.03, rng.integers(0, top + 1, (h, w)) * sign((h, w)), 0)
    elif stat == "dense":
        a = rng.integers(0, top + 1, (h, w)) * sign((h, w))
    elif stat == "constant_pos":
        a[:] = peak
    elif stat == "constant_neg":
        a[:] = -peak
    elif stat == "alternating":
        a = peak * (1 - 2 * ((xx + (yy if rng.integers(2) else 0)) & 1))
    elif stat == "checker":
        a = peak * ((xx ^ yy) & 1) * sign((h, w))
    elif stat == "runlength":
        # significant columns every fifth column; between them all-zero stripe columns, and in the middle one of each
        # gap a stripe column with a single sample at a random row of the stripe: the run-length mode and each exit
        a[:, ::5] = rng.integers(0, top + 1, (h, len(range(0, w, 5)))) * sign((h, len(range(0, w, 5))))
        for s in range(0, h, 4):
            for x in range(2, w, 5):
                if rng.integers(3):
                    y = s + int(rng.integers(4))
                    if y < h:
                        a[y, x] = int(rng.integers(1, top + 1)) * int(sign(1)[0])
    if not np.abs(a).max() >> (numbps - 1):
        a[int(rng.integers(h)), int(rng.integers(w))] = peak
    return a.astype(np.int32)


def fuzz_blocks(seed):
    """every statistic at every numbps of 1..19 and 31, sizes biased to the edges, the orientations in turn"""
    rng = np.random.default_rng(seed)
    k = 0
    for numbps in list(range(1, 20)) + [31]:
        for stat in BLOCK_STATS:
            for rep in range(2):
                w = int(rng.choice(BIASED)) if rng.integers(2) else int(rng.integers(1, 65))
                h = int(rng.choice(BIASED + [61, 62, 9, 10, 11])) if rng.integers(2) else int(rng.integers(1, 65))
                if numbps == 31 and rep:
                    w, h = 64, 64
                yield w, h, k % 4, numbps, stat, make_block(rng, w, h, numbps, stat)
                k += 1


def test_block_coder_equals_the_oracle_on_a_block_fuzz(shim):
    jp2k.counters(reset=True)
    seen = set()
    for w, h, orient, numbps, stat, a in fuzz_blocks(20261016):
        want, passes, nb = jp2k.t1_encode(a, orient)
        got, n, gp, gnb = jp2k.shim_code_block(a, orient)
        where = f"tier-1 block coder (jp2k_t1.inc): {w} x {h}, orientation {orient}, numbps {numbps}, {stat}"
        if stat == "zero":
            assert (n, gp, gnb) == (0, 0, 0) == (len(want), passes, nb), where
            continue
        assert nb == numbps, where
        assert (gnb, gp) == (nb, passes) == (numbps, 3 * numbps - 2), f"{where}: numbps / passes {gnb} / {gp}, oracle {nb} / {passes}"
        assert n == len(got) == len(want), f"{where}: {n} bytes, oracle {len(want)}"
        assert got == want, f"{where}: bytes differ from offset {next(i for i in range(n) if got[i] != want[i])} of {n}"
        assert np.array_equal(jp2k.t1_decode(got, w, h, orient, gnb, gp), a), f"{where}: the oracle's decoder does not return the block"
        seen.add((min(w, 3), h & 3, orient))
    c = jp2k.counters()
    for name in ("rl_exit0", "rl_exit1", "rl_exit2", "rl_exit3", "rl_zero", "partial_stripe", "narrow_block"):
        assert c[name] > 0, (name, c)
    assert {(ww, hh) for ww, hh, _ in seen} >= {(ww, hh) for ww in (1, 2, 3) for hh in (0, 1, 2, 3)}
    assert {o for _, _, o in seen} == {0, 1, 2, 3}


def test_block_coder_counts_beyond_its_capacity_and_writes_only_within(shim):
    rng = np.random.default_rng(99)
    for w, h, numbps, stat in [(12, 9, 9, "dense"), (1, 17, 12, "dense"), (5, 4, 19, "sparse"), (8, 8, 31, "dense"), (64, 3, 3, "checker"),
                               (2, 2, 1, "constant_neg")]:
        a = make_block(rng, w, h, numbps, stat)
        full, n, passes, nb = jp2k.shim_code_block(a, 3)
        assert len(full) == n > 0 and full == jp2k.t1_encode(a, 3)[0]
        for cap in range(n):
            part, m, p2, nb2 = jp2k.shim_code_block(a, 3, cap=cap)     # (asserts the canary behind `cap`)
            assert (m, p2, nb2) == (n, passes, nb), f"tier-1 byte clamp: cap {cap} changes the report to {(m, p2, nb2)}"
            assert part == full[:cap], f"tier-1 byte clamp: cap {cap}: not the prefix of the full result"


def random_packet(rng, k):
    nbands = 1 if rng.integers(4) == 0 else 3
    grids = [(1, 1), (1, 7), (9, 1), (3, 5), (16, 16), (2, 2), (5, 3), (16, 1), (7, 7)]
    gw, gh, mb, rec = [], [], [], []
    kind = k % 8       # 0: every block absent (an empty packet); 1: an empty band beside full ones
    for b in range(nbands):
        w, h = grids[int(rng.integers(len(grids)))] if rng.integers(2) else (int(rng.integers(1, 17)), int(rng.integers(1, 17)))
        if kind == 1 and nbands == 3 and b == k // 8 % 3:
            w, h = 0, 0
        m = int(rng.integers(9, 20))
        gw.append(w); gh.append(h); mb.append(m)
        for _ in range(w * h):
            if kind == 0 or rng.integers(5) == 0:
                rec.append((0, 0, 0))
                continue
            row = int(rng.integers(5))
            passes = int(rng.integers(*[(1, 2), (2, 3), (3, 6), (6, 37), (37, 165)][row]))
            e = int(rng.integers(0, 21))
            length = [0, 1, (1 << e) - 1, 1 << e, int(rng.integers(65536, 1 << 21)), int(rng.integers(0, 3000))][int(rng.integers(6))]
            rec.append((passes, int(rng.integers(1, m + 1)), length))
    return gw, gh, mb, np.array(rec, np.int32).reshape(-1, 3)


def test_packet_headers_equal_the_oracle_writer_and_parse_back(shim):
    rng = np.random.default_rng(410)
    jp2k.counters(reset=True)
    for k in range(400):
        gw, gh, mb, rec = random_packet(rng, k)
        want = jp2k.packet_header_write(gw, gh, mb, rec)
        got = jp2k.shim_packet_header(gw, gh, mb, rec)
        where = f"tier-2 packet header (jp2k_t2.inc put_packet_header): packet {k}, grids {list(zip(gw, gh))}"
        assert got == want, f"{where}: {got[:24].hex()}... ({len(got)} bytes), oracle {want[:24].hex()}... ({len(want)})"
        back, used = jp2k.packet_header_parse(gw, gh, mb, got + b"\x12\x34")
        assert used == len(got), where
        assert np.array_equal(back, rec), f"{where}: the oracle's parser returns other records"
    c = jp2k.counters()
    for name in ("header_stuff", "lblock_inc", "passes_16bit", "tree_not_pow2", "empty_band_beside_full", "empty_packet",
                 "excluded_in_full_packet", "pass_row0", "pass_row1", "pass_row2", "pass_row3", "pass_row4"):
        assert c[name] > 0, (name, c)


def test_block_table_equals_the_oracle_enumeration_field_by_field(shim):
    for H, W in GEOMETRIES + NEW_GEOMETRIES:
        for C, bits in ((1, 16), (3, 8)):
            o = jp2k.blocks(C, H, W, bits)
            p = jp2k.shim_blocks(C, H, W, bits)
            where = f"geometry (jp2k_t2.inc make_geometry): {C} x {H} x {W}, {bits} bits"
            assert len(o) == len(p), f"{where}: {len(p)} blocks, oracle {len(o)}"
            want = np.stack([o[:, F["tile"]] * C + o[:, F["comp"]]] + [o[:, F[k]] for k in ("x", "y", "w", "h", "orient", "mb")], 1)
            bad = np.nonzero((want != p[:, :7]).any(1))[0]
            assert not len(bad), (f"{where}: block {bad[0]} (slab, x, y, w, h, orient, mb) is {p[bad[0], :7].tolist()}, "
                                  f"oracle {want[bad[0]].tolist()}")
            assert (p[:, 3] >= 1).all() and (p[:, 4] >= 1).all() and (p[:, 3] <= 64).all() and (p[:, 4] <= 64).all()


def host_file(x):
    """the product's file without a GPU: the oracle's coefficients, the shim's block coder, the product's assemble"""
    bits = 8 * x.dtype.itemsize
    C, H, W = x.shape
    table = jp2k.shim_blocks(C, H, W, bits)
    coef, res, data = {}, np.zeros((len(table), 4), np.uint32), []
    for k, (slab, bx, by, bw, bh, orient, mb, cap) in enumerate(table.tolist()):
        if slab not in coef:
            coef[slab] = jp2k.coefficients(x, slab // C, slab % C)
        got, n, passes, nb = jp2k.shim_code_block(coef[slab][by:by + bh, bx:bx + bw], orient, cap=cap)
        assert n <= cap, f"block {k} needs {n} bytes, its slot holds {cap}"
        res[k] = (n, passes, nb, 0)
        data.append(got)
    return jp2k.shim_assemble(C, H, W, bits, res, b"".join(data))


def test_whole_files_from_the_host_text_equal_the_oracle(shim):
    cases = [(s, 16, "synth") for s in SMALL_SHAPES] + [((3, 300, 517), 8, "synth"), ((2, 100, 130), 16, "zero"),
                                                         ((2, 100, 130), 16, "mid"), ((1, 70, 70), 8, "constant"),
                                                         ((2, 257, 300), 16, "uniform"), ((1, 130, 140), 16, "spike"),
                                                         ((1, 90, 77), 16, "checker"), ((1, 90, 77), 16, "stripes_h"),
                                                         ((2, 1, 1500), 16, "synth"), ((1, 64, 1025), 8, "stripes_v")]
    for shape, bits, stat in cases:
        x = planes_of(stat, shape, bits)
        got, want = host_file(x), jp2k.encode(x)
        assert got == want, f"whole file (host text) {shape} {bits} bits {stat}: {jp2k.first_difference(got, want, x)}"
