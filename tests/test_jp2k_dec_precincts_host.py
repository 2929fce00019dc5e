"""Precinct partitions and the reversible component transform in the GPU JPEG 2000 decoder's host text
(csrc/jp2k_t2d.inc), judged on the CPU against files Pillow (OpenJPEG) wrote: tests/golden/jp2k_precincts.npz holds the
files and the samples Pillow reads back from them (tests/golden/make_golden_jp2k_precincts.py).  No GPU.  Every
comparison is exact.

The product's parser runs through tests/jp2k_dec_host_shim.cpp, compiled as tests/test_jp2k_dec_host.py compiles it.
Two things judge its block table:
  * the geometry of T.800 B.5 - B.7 and B.12 (LRCP) restated here in Python (`expected_blocks`): which blocks there are,
    in which packet order, where they lie in the Mallat slab;
  * a reconstruction without a GPU: every block of the table decoded by the product's tier-1 decoder into its slab, the
    oracle's inverse 5/3, the inverse RCT (G.2.2) and the DC shift in numpy -- the result is what Pillow reads.
tests/test_gpu_jp2k_dec_precincts.py imports the helpers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import jp2k as oracle  # noqa: E402
import make_golden_jp2k_precincts as gen  # noqa: E402
from test_jp2k_dec_host import (DEC_BAD, DEC_UNSUPPORTED, GuardedBytes, load_shim, shim_info, shim_parse, shim_t1_decode,  # noqa: E402
                                table_is_valid)
from test_jp2k_oracle import planes_of  # noqa: E402

F = oracle.F
GEOMETRY_FIELDS = ("tile", "comp", "res", "band", "gx", "gy", "mb", "x", "y", "w", "h", "orient")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


def fixture_cases(golden):
    """[(name, file bytes, [C, H, W] samples)] in the generator's order"""
    g = golden["jp2k_precincts"]
    return [(c[0], g["file_" + c[0]].tobytes(), g["planes_" + c[0]]) for c in gen.CASES]


# ------------------------------------------------------------------ the geometry, restated

def cdiv(a, b):
    return -((-a) // b)


def main_header(f):
    """what the geometry needs of SIZ, COD and QCD of a .jp2 file or raw codestream"""
    at = f.index(b"jp2c") + 4 if f[:4] != b"\xff\x4f\xff\x51" else 0
    assert f[at:at + 2] == b"\xff\x4f"
    at += 2
    h = {}
    while f[at:at + 2] != b"\xff\x90":
        n = int.from_bytes(f[at + 2:at + 4], "big")
        q = at + 4
        if f[at:at + 2] == b"\xff\x51":
            h["W"], h["H"] = int.from_bytes(f[q + 2:q + 6], "big"), int.from_bytes(f[q + 6:q + 10], "big")
            h["XT"], h["YT"] = min(int.from_bytes(f[q + 18:q + 22], "big"), h["W"]), min(int.from_bytes(f[q + 22:q + 26], "big"), h["H"])
            h["C"], h["bits"] = int.from_bytes(f[q + 34:q + 36], "big"), f[q + 36] + 1
            h["siz"] = at
        elif f[at:at + 2] == b"\xff\x52":
            h["cod"], h["scod"], h["mct"], h["NL"] = at, f[q], f[q + 4], f[q + 5]
            h["xcb"], h["ycb"] = f[q + 6] + 2, f[q + 7] + 2
            h["pp"] = [(f[q + 10 + r] & 15, f[q + 10 + r] >> 4) if f[q] & 1 else (15, 15) for r in range(h["NL"] + 1)]
        elif f[at:at + 2] == b"\xff\x5c":
            h["guard"], h["eps"] = f[q] >> 5, [b >> 3 for b in f[q + 1:at + 2 + n]]
        at += 2 + n
    h["ntx"], h["nty"] = cdiv(h["W"], h["XT"]), cdiv(h["H"], h["YT"])
    return h


def resolutions(h):
    """Per tile and non-empty resolution (B.5 - B.7): a dict with the bands (orient, bx0, by0, w, h, x, y: origin in band
    coordinates, size, place in the Mallat slab; mb), the nominal code block, and per precinct in raster order and band
    the blocks as (gx, gy, x, y, w, h) in raster order."""
    NL = h["NL"]
    for t in range(h["ntx"] * h["nty"]):
        x0, y0 = (t % h["ntx"]) * h["XT"], (t // h["ntx"]) * h["YT"]
        x1, y1 = min(x0 + h["XT"], h["W"]), min(y0 + h["YT"], h["H"])
        for r in range(NL + 1):
            s = 1 << (NL - r)
            rx0, rx1, ry0, ry1 = cdiv(x0, s), cdiv(x1, s), cdiv(y0, s), cdiv(y1, s)
            if rx1 <= rx0 or ry1 <= ry0:
                continue
            ppx, ppy = h["pp"][r]
            px0, py0 = rx0 >> ppx, ry0 >> ppy
            npx, npy = cdiv(rx1, 1 << ppx) - px0, cdiv(ry1, 1 << ppy) - py0
            ex, ey = (ppx, ppy) if r == 0 else (ppx - 1, ppy - 1)          # a precinct's span in the bands
            cw, ch = 1 << min(h["xcb"], ex), 1 << min(h["ycb"], ey)
            nb = NL if r == 0 else NL - r + 1
            bands = []
            for b, orient in enumerate([0] if r == 0 else [1, 2, 3]):
                xo, yo = orient & 1, orient >> 1
                half = (1 << (nb - 1)) if nb else 0
                bx0, bx1 = cdiv(x0 - half * xo, 1 << nb), cdiv(x1 - half * xo, 1 << nb)
                by0, by1 = cdiv(y0 - half * yo, 1 << nb), cdiv(y1 - half * yo, 1 << nb)
                bands.append(dict(orient=orient, bx0=bx0, by0=by0, w=bx1 - bx0, h=by1 - by0,
                                  x=(cdiv(rx1, 2) - cdiv(rx0, 2)) if xo else 0, y=(cdiv(ry1, 2) - cdiv(ry0, 2)) if yo else 0,
                                  mb=h["guard"] + h["eps"][0 if r == 0 else 1 + 3 * (r - 1) + b] - 1))
            precincts = []
            for py in range(npy):
                for px in range(npx):
                    per_band = []
                    for q in bands:
                        ax0, ax1 = max((px0 + px) << ex, q["bx0"]), min((px0 + px + 1) << ex, q["bx0"] + q["w"])
                        ay0, ay1 = max((py0 + py) << ey, q["by0"]), min((py0 + py + 1) << ey, q["by0"] + q["h"])
                        blocks = []
                        if ax1 > ax0 and ay1 > ay0:
                            for cy in range(ay0 // ch, cdiv(ay1, ch)):
                                for cx in range(ax0 // cw, cdiv(ax1, cw)):
                                    u0, u1 = max(cx * cw, ax0), min((cx + 1) * cw, ax1)
                                    v0, v1 = max(cy * ch, ay0), min((cy + 1) * ch, ay1)
                                    blocks.append((cx - q["bx0"] // cw, cy - q["by0"] // ch, q["x"] + u0 - q["bx0"], q["y"] + v0 - q["by0"], u1 - u0, v1 - v0))
                        per_band.append(blocks)
                    cut = ((px0 + px) << ppx) < rx0 or ((py0 + py) << ppy) < ry0        # its low side lies outside the tile
                    precincts.append(dict(bands=per_band, cut_low=cut))
            yield dict(tile=t, res=r, x0=x0, y0=y0, tw=x1 - x0, th=y1 - y0, bands=bands, cw=cw, ch=ch, npx=npx, npy=npy, precincts=precincts)


def expected_blocks(h):
    """the block table's geometry columns (GEOMETRY_FIELDS) in LRCP packet order: resolution, component, precinct, band"""
    rows = []
    per_tile = {}
    for rs in resolutions(h):
        per_tile.setdefault(rs["tile"], []).append(rs)
    for t in sorted(per_tile):
        for rs in per_tile[t]:
            for c in range(h["C"]):
                for pr in rs["precincts"]:
                    for b, blocks in enumerate(pr["bands"]):
                        q = rs["bands"][b]
                        rows += [(t, c, rs["res"], b, gx, gy, q["mb"], x, y, w, hh, q["orient"]) for gx, gy, x, y, w, hh in blocks]
    return np.array(rows, np.int64).reshape(-1, len(GEOMETRY_FIELDS))


# ------------------------------------------------------------------ reconstruction without a GPU

def inverse_rct(y):
    """T.800 G.2.2 on [3, ...] integers; the floor is numpy's floor division"""
    i1 = y[0] - (y[1] + y[2]) // 4
    return np.stack([y[2] + i1, i1, y[1] + i1])


def forward_rct(i):
    """T.800 G.2.1"""
    return np.stack([(i[0] + 2 * i[1] + i[2]) // 4, i[2] - i[1], i[0] - i[1]])


def reconstruct(L, f, rec=None):
    """the file's samples [C, H, W] from the product's block table: tier-1 by the product's decoder (through the shim),
    the inverse 5/3 by the oracle, inverse RCT and DC shift in numpy"""
    h = main_header(f)
    if rec is None:
        rc, rec = shim_parse(L, f)
        assert rc == 0, rec
    C, NL, bits = h["C"], h["NL"], h["bits"]
    out = np.zeros((C, h["H"], h["W"]), np.int64)
    room = GuardedBytes(max(int(rec[:, F["length"]].max()), 1))
    for t in range(h["ntx"] * h["nty"]):
        x0, y0 = (t % h["ntx"]) * h["XT"], (t // h["ntx"]) * h["YT"]
        tw, th = min(h["XT"], h["W"] - x0), min(h["YT"], h["H"] - y0)
        slabs = np.zeros((C, th, tw), np.int32)
        for r in rec[rec[:, F["tile"]] == t]:
            if r[F["passes"]]:
                c, bx, by, bw, bh = (int(r[F[k]]) for k in ("comp", "x", "y", "w", "h"))
                data = f[r[F["offset"]]:r[F["offset"]] + r[F["length"]]]
                slabs[c, by:by + bh, bx:bx + bw] = shim_t1_decode(L, room, data, bw, bh, int(r[F["orient"]]), int(r[F["numbps"]]), int(r[F["passes"]]))
        v = np.stack([oracle.dwt53(slabs[c], NL, x0, y0, inverse=True) for c in range(C)]).astype(np.int64)
        if h["mct"]:
            v[:3] = inverse_rct(v[:3])
        out[:, y0:y0 + th, x0:x0 + tw] = v
    return np.clip(out + (1 << (bits - 1)), 0, (1 << bits) - 1).astype(np.uint8 if bits <= 8 else np.uint16)


def describe_difference(h, got, want):
    """'' or a sentence naming the first differing component, tile and sample"""
    if np.array_equal(got, want):
        return ""
    c, y, x = (int(v) for v in np.argwhere(got != want)[0])
    t = (y // h["YT"]) * h["ntx"] + x // h["XT"]
    return (f"{int((got != want).sum())} samples differ, first in component {c}, tile {t} at sample (y {y}, x {x}): {int(got[c, y, x])}, expected "
            f"{int(want[c, y, x])}" + (f"; component {c} passes through the inverse RCT (mct = 1)" if h["mct"] and c < 3 else "; no component transform on this component"))


def test_every_fixture_file_reconstructs_to_what_pillow_reads(shim, golden):
    cases = fixture_cases(golden)
    assert len(cases) == 6
    for name, f, want in cases:
        rc, i = shim_info(shim, f)
        assert rc == 0, f"{name}: refused with {rc}: {i}"
        assert (i["C"], i["H"], i["W"]) == want.shape and i["bits"] == (8 if want.dtype == np.uint8 else 16), (name, i)
        got = reconstruct(shim, f)
        assert got.dtype == want.dtype
        assert not describe_difference(main_header(f), got, want), f"{name}: {describe_difference(main_header(f), got, want)}"


# ------------------------------------------------------------------ the table

def assert_table_invariants(name, h, rec, f):
    """table_is_valid, rectangles inside the slab, blocks pairwise disjoint and tiling every band exactly, the bytes of
    included blocks disjoint and inside the tile-parts (behind the first SOD, before EOC)"""
    assert table_is_valid(rec, len(f)), name
    for rs in resolutions(h):
        mine = rec[(rec[:, F["tile"]] == rs["tile"]) & (rec[:, F["res"]] == rs["res"])]
        for c in range(h["C"]):
            cover = np.zeros((rs["th"], rs["tw"]), np.int32)
            for r in mine[mine[:, F["comp"]] == c]:
                x, y, w, hh = (int(r[F[k]]) for k in ("x", "y", "w", "h"))
                q = rs["bands"][int(r[F["band"]])]
                assert q["x"] <= x and x + w <= q["x"] + q["w"] and q["y"] <= y and y + hh <= q["y"] + q["h"], (name, "a block outside its band", r)
                cover[y:y + hh, x:x + w] += 1
            want = np.zeros_like(cover)
            for q in rs["bands"]:
                want[q["y"]:q["y"] + q["h"], q["x"]:q["x"] + q["w"]] += 1
            assert np.array_equal(cover, want), f"{name}: tile {rs['tile']}, resolution {rs['res']}, component {c}: the blocks do not tile the bands exactly"
    inc = rec[rec[:, F["passes"]] > 0]
    order = np.argsort(inc[:, F["offset"]], kind="stable")
    lo, hi = inc[order, F["offset"]], inc[order, F["offset"]] + inc[order, F["length"]]
    assert (lo[1:] >= hi[:-1]).all(), f"{name}: byte ranges of two blocks overlap"
    first_sod = f.index(b"\xff\x93", f.index(b"\xff\x90", h["cod"]))
    assert len(inc) == 0 or (lo[0] >= first_sod + 2 and hi[-1] <= len(f) - 2), name


def test_table_equals_the_restated_geometry_and_keeps_its_invariants_on_every_file(shim, golden):
    cols = [F[k] for k in GEOMETRY_FIELDS]
    for name, f, _ in fixture_cases(golden):
        h = main_header(f)
        rc, rec = shim_parse(shim, f)
        assert rc == 0, (name, rec)
        want = expected_blocks(h)
        assert rec.shape[0] == want.shape[0], f"{name}: {len(rec)} blocks, the geometry has {len(want)}"
        bad = np.flatnonzero((rec[:, cols] != want).any(axis=1))
        assert not len(bad), f"{name}: block {bad[0]}: {dict(zip(GEOMETRY_FIELDS, rec[bad[0], cols]))}, the geometry has {dict(zip(GEOMETRY_FIELDS, want[bad[0]]))}"
        assert_table_invariants(name, h, rec, f)
        rc, i = shim_info(shim, f)
        assert rc == 0 and i["blocks"] == len(want) and i["tiles"] == h["ntx"] * h["nty"] and i["resolutions"] == h["NL"] + 1


def test_a_file_without_a_partition_keeps_the_oracles_table(shim):
    """the walk over precincts is the walk of before where COD announces none (one precinct per resolution)"""
    for shape in ((2, 90, 130), (1, 1030, 70)):
        f = oracle.encode(planes_of("synth", shape, 16))
        rc, rec = shim_parse(shim, f)
        assert rc == 0 and np.array_equal(rec, oracle.parse(f))
        assert np.array_equal(rec[:, [F[k] for k in GEOMETRY_FIELDS]], expected_blocks(main_header(f)))


def test_the_fixture_exercises_what_it_is_there_for(shim, golden):
    n = dict(many=0, some_band_empty=0, all_bands_empty=0, small=0, cut=0, narrowed=0, zero_exponent=0)
    for name, f, _ in fixture_cases(golden):
        h = main_header(f)
        for rs in resolutions(h):
            n["many"] += rs["npx"] * rs["npy"] > 1
            n["narrowed"] += rs["cw"] < (1 << h["xcb"]) or rs["ch"] < (1 << h["ycb"])
            n["zero_exponent"] += rs["res"] == 0 and h["pp"][0] == (0, 0)
            for pr in rs["precincts"]:
                counts = [len(b) for b in pr["bands"]]
                n["some_band_empty"] += h["C"] * (min(counts) == 0)
                n["all_bands_empty"] += h["C"] * (max(counts) == 0)
                n["cut"] += pr["cut_low"]
                if rs["cw"] < 4 and rs["ch"] < 4:
                    n["small"] += h["C"] * sum(counts)
    print("precinct fixture coverage:", n)
    assert n["many"] > 0, "no resolution with more than one precinct"
    assert n["some_band_empty"] > 0, "no packet of a precinct that holds no block in some band"
    assert n["all_bands_empty"] > 0, "no packet of a precinct that holds no block at all"
    assert n["small"] > 0, "no block smaller than 4 x 4"
    assert n["cut"] > 0, "no precinct cut by a tile edge"
    assert n["narrowed"] > 0 and n["zero_exponent"] > 0


# ------------------------------------------------------------------ refusals

def patched(f, pos, value):
    b = bytearray(f)
    b[pos] = value
    return bytes(b)


def with_marker_before_cod(f, h, marker):
    at = f.index(b"jp2c") + 4
    data = f[:h["cod"]] + marker + b"\x00\x04\x00\x00" + f[h["cod"]:]
    return data[:at - 8] + (len(data) - at + 8).to_bytes(4, "big") + data[at - 4:]


def test_pinned_refusals(shim, golden):
    f = oracle.encode(planes_of("synth", (2, 90, 130), 16))
    h = main_header(f)
    cod, siz = h["cod"], h["siz"]
    # the partition bit without the size bytes; the transform on two components
    for what, data, code, word in (("Scod bit 0 alone", patched(f, cod + 4, 1), DEC_UNSUPPORTED, "precinct"),
                                   ("mct on two components", patched(f, cod + 8, 1), DEC_UNSUPPORTED, "component transform"),
                                   ("RLCP", patched(f, cod + 5, 1), DEC_UNSUPPORTED, "progression"),
                                   ("two layers", patched(f, cod + 7, 2), DEC_UNSUPPORTED, "layers"),
                                   ("bypass style", patched(f, cod + 12, 1), DEC_UNSUPPORTED, "style"),
                                   ("9/7", patched(f, cod + 13, 0), DEC_UNSUPPORTED, "9/7"),
                                   ("signed", patched(f, siz + 40, 0x8F), DEC_UNSUPPORTED, "signed"),
                                   ("sub-sampled", patched(f, siz + 41, 2), DEC_UNSUPPORTED, "sub-sampled")):
        for call in (shim_info, shim_parse):
            rc, msg = call(shim, data)
            assert rc == code and word in msg, (what, rc, msg)
    for marker, word in ((b"\xff\x60", "PPM"), (b"\xff\x53", "COC"), (b"\xff\x5d", "QCC"), (b"\xff\x5e", "RGN"), (b"\xff\x5f", "POC")):
        rc, msg = shim_info(shim, with_marker_before_cod(f, h, marker))
        assert rc == DEC_UNSUPPORTED and word in msg, (marker.hex(), rc, msg)
    # the same on files WITH a partition and the transform: what is out of scope stays refused
    cases = fixture_cases(golden)
    for name, g, _ in (cases[0], cases[2]):
        k = main_header(g)
        for what, data, word in (("RLCP", patched(g, k["cod"] + 5, 1), "progression"), ("RPCL", patched(g, k["cod"] + 5, 2), "progression"),
                                 ("two layers", patched(g, k["cod"] + 7, 2), "layers"), ("style", patched(g, k["cod"] + 12, 4), "style"),
                                 ("9/7", patched(g, k["cod"] + 13, 0), "9/7"), ("signed", patched(g, k["siz"] + 40, 0x87), "signed")):
            rc, msg = shim_info(shim, data)
            assert rc == DEC_UNSUPPORTED and word in msg, (name, what, rc, msg)
        sot = g.index(b"\xff\x90", k["cod"])
        ppt = g[:sot + 12] + b"\xff\x61\x00\x03\x00" + g[sot + 12:]
        rc, msg = shim_info(shim, ppt)
        assert rc in (DEC_UNSUPPORTED, DEC_BAD) and msg       # (Psot no longer fits: refused either as PPT or as a damaged tile-part)
    # a precinct exponent of 0 above the lowest resolution is a damaged file; a partition of more precincts than the cap
    # is refused before anything is allocated for it
    name, g, _ = cases[1]
    k = main_header(g)
    assert k["pp"][0] == (0, 0)
    rc, msg = shim_info(shim, patched(g, k["cod"] + 14 + 2, 0x20))
    assert rc == DEC_BAD and "precinct" in msg, (rc, msg)
    big = bytearray(g)
    for off in (2, 6, 18, 22):                                 # Xsiz, Ysiz, XTsiz, YTsiz: 65536 -- 2048 x 2048 precincts of 1 x 1 at r = 0
        big[k["siz"] + 4 + off:k["siz"] + 8 + off] = (65536).to_bytes(4, "big")
    for call in (shim_info, shim_parse):
        rc, msg = call(shim, bytes(big))
        assert rc == DEC_UNSUPPORTED and "precinct" in msg, (rc, msg)


# ------------------------------------------------------------------ robustness

def smallest_two(golden):
    return sorted(fixture_cases(golden), key=lambda c: len(c[1]))[:2]


def truncations(f, count):
    return [f[:int(c)] for c in np.linspace(0, len(f) - 1, count).astype(int)]


def corruptions(L, f, count, seed=11):
    """single-byte corruptions of everything that is not block data (the intact file's own table says where that is)"""
    rc, rec = shim_parse(L, f)
    assert rc == 0
    is_data = np.zeros(len(f), bool)
    for r in rec[rec[:, F["passes"]] > 0]:
        is_data[r[F["offset"]]:r[F["offset"]] + r[F["length"]]] = True
    where = np.flatnonzero(~is_data)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(f)
        b[int(where[int(rng.integers(len(where)))])] ^= int(rng.integers(1, 256)) if k % 3 else (1 << int(rng.integers(8)))
        out.append(bytes(b))
    return out


def check_damaged(L, name, data, room):
    """an error, or a table the device can rely on (table_is_valid and every rectangle inside the slab of the geometry the
    parser itself reports); never a read behind the buffer (the guard page).  Returns the table or None."""
    rc, got = shim_parse(L, data, room=room)
    if rc:
        assert rc in (DEC_BAD, DEC_UNSUPPORTED) and got, (name, rc, got)
        return None
    assert table_is_valid(got, len(data)), name
    rc, i = shim_info(L, data, room=room)
    assert rc == 0 and i["blocks"] == len(got), (name, rc, i)
    tw, th = min(i["tw"], i["W"]), min(i["th"], i["H"])
    assert (got[:, F["x"]] >= 0).all() and (got[:, F["y"]] >= 0).all(), name
    assert (got[:, F["x"]] + got[:, F["w"]] <= tw).all() and (got[:, F["y"]] + got[:, F["h"]] <= th).all(), name
    assert (got[:, F["tile"]] < i["tiles"]).all() and (got[:, F["comp"]] < i["C"]).all(), name
    return got


def test_truncated_and_corrupted_precinct_files_end_in_an_error_or_a_valid_table(shim, golden):
    for name, f, _ in smallest_two(golden):
        room = GuardedBytes(len(f))
        assert check_damaged(shim, name, f, room) is not None
        errors = tables = 0
        for data in truncations(f, 200):
            got = check_damaged(shim, f"{name} cut to {len(data)}", data, room)
            assert got is None, f"{name} cut to {len(data)} of {len(f)} bytes still parses"
        for k, data in enumerate(corruptions(shim, f, 500)):
            got = check_damaged(shim, f"{name} corruption {k}", data, room)
            errors += got is None
            tables += got is not None
        print(f"{name}: {len(f)} bytes, 200 truncations refused, 500 corruptions: {errors} refused, {tables} parsed to a valid table")
        assert errors > 0


# ------------------------------------------------------------------ the writer, live

def test_pillow_writes_the_fixtures_files_today(shim, golden):
    try:
        import PIL
        from PIL import features
    except ImportError:
        pytest.skip("Pillow is not importable: the fixture's files cannot be regenerated here")
    if not features.check_codec("jpg_2000"):
        pytest.skip("this Pillow has no JPEG 2000 codec: the fixture's files cannot be regenerated here")
    g = golden["jp2k_precincts"]
    same_writer = (str(g["pillow_version"]), str(g["openjpeg_version"])) == (PIL.__version__, str(features.version_codec("jpg_2000")))
    for k, (name, f, want) in enumerate(fixture_cases(golden)):
        live, back = gen.write_case(k)             # (asserts Pillow's own round trip, the partition bit and mct)
        assert np.array_equal(back, want), name
        if same_writer:
            assert live == f, f"{name}: Pillow {PIL.__version__} writes other bytes than the fixture holds"
        else:                                      # another OpenJPEG may order or terminate differently: its file must decode all the same
            assert np.array_equal(reconstruct(shim, live), want), name
    if not same_writer:
        print(f"fixture written by Pillow {g['pillow_version']} / OpenJPEG {g['openjpeg_version']}, this is {PIL.__version__} / "
              f"{features.version_codec('jpg_2000')}: bytes not compared, the live files were decoded instead")
