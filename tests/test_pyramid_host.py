"""The overview pyramid on the CPU: tests/pyramid_reference.py against the worked example of the definition and against a
brute-force evaluation in Python integers; the host build of csrc/pyramid.inc (tests/pyramid_host_shim.cpp, g++: the
per-sample text the device runs) against the reference on every level of the shapes of tests/pyramid_helpers.py; the level
rule; the library's checks that come before any launch; the container of a pyramidal file (tiff_write.assemble_pyramid) read
by an IFD walker of this file's own; whole files, built from the host builds of the pyramid and of the writer, read by Pillow
and by tiff.parse(ifd=k) with the reference decoders; the georeferencing tags; the command lines' refusals; the kernels'
resource usage; and tests/pyramid_main.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer.  No GPU.  Every comparison is exact: the reduction is integer arithmetic."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_helpers as H  # noqa: E402
import tiff_write_helpers as TW  # noqa: E402
from pyramid_helpers import CSRC, ROOT  # noqa: E402

R = H.R


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return H.load_shim(tmp_path_factory)


@pytest.fixture(scope="module")
def tiffw_shim(tmp_path_factory):
    return TW.load_shim(tmp_path_factory)


# ---------------------------------------------------------------- the reference itself

def test_reference_gives_the_worked_example_and_equals_a_brute_force_evaluation():
    assert np.array_equal(R.reduce_level(H.EXAMPLE), H.EXAMPLE_LEVEL)
    assert np.array_equal(R.reduce_level(H.EXAMPLE, "nearest"), [[[0, 65535], [65535, 65534]]])
    for dtype in (np.uint8, np.uint16):
        a = H.raster((2, 7, 9), dtype, "random", None)
        A = a.tolist()
        for nodata in H.nodatas(dtype):
            got = R.reduce_level(a, "average", nodata)
            assert got.shape == (2, 4, 5) and got.dtype == a.dtype
            seen = set()
            for c in range(2):
                for y in range(4):
                    for x in range(5):
                        vals = [A[c][2 * y + dy][2 * x + dx] for dy in (0, 1) for dx in (0, 1) if 2 * y + dy < 7 and 2 * x + dx < 9]
                        vals = [v for v in vals if v != nodata]
                        seen.add(len(vals))
                        want = (2 * sum(vals) + len(vals)) // (2 * len(vals)) if vals else nodata      # round half up, another way
                        assert got[c, y, x] == want
            assert seen >= ({1, 2, 4} if nodata is None else {0, 1, 2, 3, 4})
    # a cascade: level 2 is the reduction of level 1, not of the raster
    a = H.raster((1, 9, 9), np.uint16, "random", None)
    lv = R.pyramid(a, 4, "average", 0)
    assert [v.shape for v in lv] == [(1, 5, 5), (1, 3, 3), (1, 2, 2), (1, 1, 1)] and np.array_equal(lv[1], R.reduce_level(lv[0], "average", 0))
    with pytest.raises(ValueError):
        R.pyramid(a, 5)


# ---------------------------------------------------------------- the host build against the reference

@pytest.mark.parametrize("shape", H.SHAPES, ids=H.shape_id)
def test_host_build_equals_reference_on_every_level(shim, shape):
    n = 0
    for dtype, resampling, nodata, data, a, want in H.cases(shape):
        got = H.shim_build(shim, a, len(want), resampling, nodata)
        assert len(got) == len(want) == R.max_levels(*shape[1:]) and got[-1].shape == (shape[0], 1, 1)
        for k, (g, w) in enumerate(zip(got, want), 1):
            assert g.shape == w.shape and np.array_equal(g, w), (shape, np.dtype(dtype).name, resampling, nodata, data, k)
        if data == "all nodata" and nodata is not None and resampling == "average":
            assert all((g == nodata).all() for g in got)
        if data == "all maximum" and nodata != H.top_of(dtype):
            assert all((g == H.top_of(dtype)).all() for g in got)      # sums of four maxima need more than 16 bits
        n += 1
    assert n == 2 * 3 * 3 * 2
    if shape == (1, 3, 3):
        assert np.array_equal(H.shim_build(shim, H.EXAMPLE, 1)[0], H.EXAMPLE_LEVEL)


def test_host_build_reduces_a_window_where_it_lies_and_fewer_levels_are_a_prefix(shim):
    for dtype in (np.uint8, np.uint16):
        scene = H.raster((3, 40, 61), dtype, "random", None)
        for view in ((3, 5, 20, 31), (0, 1, 40, 33), (17, 8, 13, 53)):
            y0, x0, h, w = view
            crop = np.ascontiguousarray(scene[:, y0:y0 + h, x0:x0 + w])
            for resampling in H.RESAMPLINGS:
                want = R.pyramid(crop, 3, resampling, 0)
                got = H.shim_build(shim, scene, 3, resampling, 0, view=view)
                assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))
                assert all(np.array_equal(g, w_) for g, w_ in zip(H.shim_build(shim, crop, 2, resampling, 0), want[:2]))


def test_rounded_mean_is_round_half_up_for_every_count_and_sum(shim):
    for n in (1, 2, 3, 4):
        for s in list(range(0, 64)) + list(range(n * 65535 - 40, n * 65535 + 1)):
            assert shim.pyr_shim_rounded_mean(s, n) == (s + n // 2) // n == (2 * s + n) // (2 * n)


# ---------------------------------------------------------------- the level rule

def test_level_rule_and_level_sizes(shim):
    from lbdrn_hip import pyramid
    L = pyramid.lib()
    assert pyramid.level_sizes(6000, 6000, "auto") == pyramid.level_sizes(6000, 6000, "auto", 256) == \
        [(3000, 3000), (1500, 1500), (750, 750), (375, 375), (188, 188)]
    assert pyramid.level_sizes(7550, 7550, "auto", 256) == [(3775, 3775), (1888, 1888), (944, 944), (472, 472), (236, 236)]
    assert pyramid.level_sizes(75, 130, "auto", 16) == [(38, 65), (19, 33), (10, 17), (5, 9)]
    assert pyramid.level_sizes(37, 53, "auto", (16, 32)) == [(19, 27)]
    assert pyramid.level_sizes(256, 256, "auto", 256) == pyramid.level_sizes(16, 9, "auto", 16) == pyramid.level_sizes(40, 40, None) == []
    assert pyramid.level_sizes(257, 1, "auto", 256) == [(129, 1)]
    assert pyramid.level_sizes(5, 130, 8) == [(3, 65), (2, 33), (1, 17), (1, 9), (1, 5), (1, 3), (1, 2), (1, 1)]
    assert pyramid.level_sizes(5, 130, "3") == pyramid.level_sizes(5, 130, 3) and pyramid.level_sizes(5, 130, 0) == []
    for bad in (9, "9"):
        with pytest.raises(ValueError, match="1 x 1"):
            pyramid.level_sizes(5, 130, bad)
    with pytest.raises(ValueError, match="1 x 1"):
        pyramid.level_sizes(1, 1, 1)
    for bad in (-1, "many", 1.5, True):
        with pytest.raises(ValueError, match="overviews"):
            pyramid.level_sizes(40, 40, bad)
    hk, wk = ctypes.c_int32(), ctypes.c_int32()
    for Hh, W in ((6000, 6000), (7550, 7550), (75, 130), (5, 130), (1, 2), (2, 1), (1, 200), (64, 64), (65, 129), (1, 1), (1 << 20, 3)):
        for tile in (16, 256):
            want = R.level_sizes(Hh, W, "auto", tile)
            assert pyramid.level_sizes(Hh, W, "auto", tile) == want
            assert L.lbdrn_pyr_level_count(Hh, W, tile) == shim.pyr_shim_level_count(Hh, W, tile) == len(want)
            assert not want or max(want[-1]) <= tile < max(([(Hh, W)] + want)[-2])      # the last level is the first that fits one tile
        top = R.max_levels(Hh, W)
        assert pyramid.max_levels(Hh, W) == shim.pyr_shim_max_levels(Hh, W) == top
        sizes = [(Hh, W)] + R.level_sizes(Hh, W, top)
        assert sizes[-1] == (1, 1) and (top == 0 or sizes[-2] != (1, 1))
        for k, (h, w) in enumerate(sizes):
            assert L.lbdrn_pyr_level_size(Hh, W, k, ctypes.byref(hk), ctypes.byref(wk)) == 0 and (hk.value, wk.value) == (h, w)
        assert L.lbdrn_pyr_level_size(Hh, W, top + 1, ctypes.byref(hk), ctypes.byref(wk)) == pyramid.E_ARG
        assert b"no level" in L.lbdrn_pyr_last_error()
    assert L.lbdrn_pyr_level_count(0, 5, 16) == L.lbdrn_pyr_level_count(5, 5, 0) == pyramid.E_ARG


def test_output_layout_levels_back_to_back_each_on_256_bytes(shim):
    from lbdrn_hip import pyramid
    L = pyramid.lib()
    for (C, Hh, W) in H.SHAPES + ((8, 6000, 6000),):
        for bits in (8, 16):
            d = pyramid.Desc(C, Hh, W, bits, 0, 0, 0, 0, W, Hh * W)
            at = 0
            for k, (h, w) in enumerate(R.level_sizes(Hh, W, R.max_levels(Hh, W)), 1):
                assert L.lbdrn_pyr_level_offset(ctypes.byref(d), k) == shim.pyr_shim_level_offset(C, Hh, W, k, bits // 8) == at
                end = at + C * h * w * bits // 8
                assert L.lbdrn_pyr_output_bytes(ctypes.byref(d), k) == shim.pyr_shim_output_bytes(C, Hh, W, k, bits // 8) == end
                at = -(-end // 256) * 256
            assert L.lbdrn_pyr_output_bytes(ctypes.byref(d), 0) == L.lbdrn_pyr_output_bytes(ctypes.byref(d), k + 1) == 0
            assert L.lbdrn_pyr_level_offset(ctypes.byref(d), 0) == L.lbdrn_pyr_level_offset(ctypes.byref(d), k + 1) == 0
    assert L.lbdrn_pyr_output_bytes(None, 1) == 0
    assert L.lbdrn_pyr_output_bytes(ctypes.byref(pyramid.Desc(0, 5, 5, 16, 0, 0, 0, 0, 5, 25)), 1) == 0


# ---------------------------------------------------------------- the library's checks that come before any launch

def test_library_refuses_before_any_launch():
    from lbdrn_hip import pyramid
    L = pyramid.lib()
    assert L.lbdrn_pyr_abi_version() == 1
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before any device work
    C, Hh, W = 8, 75, 130
    good = dict(C=C, H=Hh, W=W, bits=16, resampling=0, has_nodata=0, nodata=0, reserved=0, row_pitch=W, plane_pitch=Hh * W)
    need = L.lbdrn_pyr_output_bytes(ctypes.byref(pyramid.Desc(**good)), 4)
    assert need > 0

    def call(src=fake, out=fake, levels=4, out_bytes=need, desc=True, **kw):
        d = pyramid.Desc(**dict(good, **kw))
        return L.lbdrn_pyr_build(ctypes.byref(d) if desc else None, src, levels, out, out_bytes, None)
    err = L.lbdrn_pyr_last_error
    for kw in (dict(src=None), dict(out=None), dict(desc=False)):
        assert call(**kw) == pyramid.E_ARG and b"null" in err()
    for kw in (dict(C=0), dict(H=0), dict(W=0), dict(C=-3), dict(C=65536), dict(H=(1 << 20) + 1), dict(H=1 << 20, W=4096, row_pitch=4096)):
        assert call(**kw) == pyramid.E_ARG and b"out of range" in err()
    for bits in (0, -8, 33, 64):
        assert call(bits=bits) == pyramid.E_ARG and b"bit samples are out of range" in err()
    assert call(row_pitch=W - 1) == pyramid.E_ARG and b"row pitch" in err()
    assert call(plane_pitch=-1) == pyramid.E_ARG and b"plane pitch" in err()
    assert call(has_nodata=2) == pyramid.E_ARG and b"has_nodata" in err()
    assert call(has_nodata=1, nodata=65536) == pyramid.E_ARG and b"nodata" in err()
    assert call(has_nodata=1, nodata=256, bits=8) == pyramid.E_ARG and b"nodata" in err()
    for levels in (0, -1, 9):
        assert call(levels=levels) == pyramid.E_ARG and b"1 x 1" in err()
    assert call(src=ctypes.c_void_p(4097)) == pyramid.E_ARG and b"aligned" in err()
    assert call(out=ctypes.c_void_p(4097)) == pyramid.E_ARG and b"aligned" in err()
    assert call(out_bytes=need - 1) == pyramid.E_ARG and b"levels need" in err()
    assert call(out_bytes=0) == pyramid.E_ARG
    # what is not built, after every argument has passed
    for bits in (1, 12, 32):
        assert call(bits=bits, out_bytes=1 << 40) == pyramid.E_UNSUPPORTED and b"8 and 16" in err()
    for resampling in (2, -1):
        assert call(resampling=resampling) == pyramid.E_UNSUPPORTED and b"resampling" in err()
    # precedence: LBDRN_E_ARG first
    assert call(bits=12, out_bytes=0) == pyramid.E_ARG and b"levels need" in err()
    assert call(resampling=2, levels=9) == pyramid.E_ARG
    assert call(bits=12, resampling=2, out_bytes=1 << 40) == pyramid.E_UNSUPPORTED and b"8 and 16" in err()      # bits before resampling


def test_python_refuses_before_any_device_work(tmp_path):
    import torch
    from lbdrn_hip import pyramid, raster_io, tiff_write
    t = torch.zeros((2, 20, 30), dtype=torch.int16)
    for kw, word in ((dict(levels=0), "levels"), (dict(levels=6), "1 x 1"), (dict(levels=1, resampling="bilinear"), "resampling"),
                     (dict(levels=1, nodata=65536), "nodata"), (dict(levels=1, nodata=-1), "nodata"), (dict(levels=1, nodata=0.5), "nodata")):
        with pytest.raises(ValueError, match=word):
            pyramid.build(t, **kw)
    with pytest.raises(ValueError, match="nodata"):
        pyramid.build(torch.zeros((2, 20, 30), dtype=torch.uint8), 1, nodata=256)
    for bad in (torch.zeros((20, 30), dtype=torch.int16), torch.zeros((2, 20, 30), dtype=torch.float32), np.zeros((2, 20, 30), np.uint16)):
        with pytest.raises(ValueError, match="C,H,W"):
            pyramid.build(bad, 1)
    with pytest.raises(pyramid.PyramidError, match="GPU"):
        pyramid.build(t, 1)      # a host tensor
    a = np.zeros((2, 20, 30), np.uint16)
    tif, npy = str(tmp_path / "a.tif"), str(tmp_path / "a.npy")
    for kw, word in ((dict(overviews="auto", rows_per_strip=8), "overviews go with tiles"), (dict(overviews=6), "1 x 1"),
                     (dict(overviews="some"), "overviews"), (dict(overviews=1, resampling="cubic"), "resampling"),
                     (dict(nodata=0), "overviews"), (dict(overviews=1, nodata=70000), "nodata")):
        for write in (raster_io.write_raster, tiff_write.write):
            with pytest.raises(ValueError, match=word):
                write(tif, a, **kw)
        with pytest.raises(ValueError, match=word):
            raster_io.write_raster_device(tif, t, **kw)
    for kw in (dict(overviews=1), dict(nodata=0), dict(resampling="nearest"), dict(geo=H.GEO)):
        with pytest.raises(ValueError, match="not of a .npy"):
            raster_io.write_raster(npy, a, **kw)
        with pytest.raises(ValueError, match="not of a .npy"):
            raster_io.write_raster_device(npy, t, compress=None, **kw)
    assert not os.path.exists(tif) and not os.path.exists(npy)
    np.save(npy, a)
    with pytest.raises(IndexError, match="no overview"):
        raster_io.read_raster(npy, overview=1)
    with pytest.raises(ValueError, match="overview"):
        raster_io.read_raster(npy, overview=-1)
    assert raster_io.read_geo_tags(npy) == []
    # bad geo entries
    lay = tiff_write.make_layout(1, 20, 30, 16, "deflate", 16, cap=1 << 20)
    for geo, word in (([(256, 3, 1, b"\0\0")], "sets itself"), ([(34735, 3, 2, b"\0\0")], "value bytes"), ([(34735, 99, 1, b"\0")], "value bytes"),
                      ([H.GEO[0], H.GEO[0]], "twice"), ([(34735, 3)], "no \\(tag")):
        with pytest.raises(ValueError, match=word):
            tiff_write.assemble_pyramid([lay], [[1] * 4], geo)


# ---------------------------------------------------------------- the container, read by a walker of this file's own

def walk(buf):
    """[(IFD offset, {tag: (type, count, values or bytes)}, end of the IFD and of its out-of-line values)] along the chain, and
    whether the file is a BigTIFF; little-endian files only"""
    assert buf[:2] == b"II"
    big = struct.unpack_from("<H", buf, 2)[0] == 43
    assert big or struct.unpack_from("<H", buf, 2)[0] == 42
    off = struct.unpack_from("<Q", buf, 8)[0] if big else struct.unpack_from("<I", buf, 4)[0]
    size = {1: 1, 2: 1, 3: 2, 4: 4, 12: 8, 16: 8}
    code = {3: "H", 4: "I", 16: "Q"}
    out = []
    while off:
        assert off % 2 == 0 and len(out) < 64
        n = struct.unpack_from("<Q" if big else "<H", buf, off)[0]
        p = off + (8 if big else 2)
        tags, end, last = {}, p + n * (20 if big else 12) + (8 if big else 4), 0
        for i in range(n):
            tag, typ = struct.unpack_from("<HH", buf, p)
            cnt = struct.unpack_from("<Q" if big else "<I", buf, p + 4)[0]
            assert tag > last, "tags are in ascending order"
            last = tag
            vp, nbytes = p + (12 if big else 8), size[typ] * cnt
            if nbytes > (8 if big else 4):
                vp = struct.unpack_from("<Q" if big else "<I", buf, vp)[0]
                assert vp % 2 == 0 and vp >= end - 0, "out-of-line values follow their IFD"
                end = max(end, vp + nbytes)
            raw = bytes(buf[vp:vp + nbytes])
            assert len(raw) == nbytes
            tags[tag] = (typ, cnt, list(struct.unpack("<%d%s" % (cnt, code[typ]), raw)) if typ in code else raw)
            p += 20 if big else 12
        out.append((off, tags, end))
        off = struct.unpack_from("<Q" if big else "<I", buf, p)[0]
    return out, big


def _layouts(C, Hh, W, bits, levels, tile=16, planar=2):
    from lbdrn_hip import tiff_write
    sizes = [(Hh, W)] + R.level_sizes(Hh, W, levels)
    return [tiff_write.make_layout(C, h, w, bits, "deflate", tile, None, planar, None, cap=1 << 20) for h, w in sizes]


@pytest.mark.parametrize("nlevels", (0, 1, 3, 5))
@pytest.mark.parametrize("fake", (None, (1 << 32) - 20000, 1 << 32), ids=("real", "classic to the brim", "bigtiff"))
def test_container_chain_tables_and_data_order(nlevels, fake):
    from lbdrn_hip import tiff_write
    lays = _layouts(3, 75, 130, 16, nlevels)
    rng = np.random.default_rng(nlevels)
    counts = [rng.integers(1, 400, tiff_write.segment_count(lay)).tolist() for lay in lays]
    bodies = [sum(c) for c in counts]
    if fake is not None:
        bodies[0] = fake - sum(bodies[1:])      # the full resolution is as large as it takes; its segments are still where the table says
    geo = H.GEO if nlevels != 1 else None
    head, offsets = tiff_write.assemble_pyramid(lays, counts, geo, body_bytes=bodies)
    ifds, big = walk(head)
    assert big == (fake == 1 << 32)
    assert len(ifds) == nlevels + 1 and len(offsets) == nlevels + 1
    first_data = min(min(o) for o in offsets)
    assert first_data == len(head)
    spans = []
    for k, ((off, tags, end), lay) in enumerate(zip(ifds, lays)):
        assert end <= first_data, "every IFD and table lies in front of the first segment byte"
        assert (tags.get(254, (0, 0, [0]))[2] == [1]) == (k > 0) and (254 in tags) == (k > 0)
        assert tags[256][2] == [lay.W] and tags[257][2] == [lay.H] and tags[258][2] == [16] * 3 and tags[277][2] == [3]
        assert tags[259][2] == [8] and tags[317][2] == [2] and tags[284][2] == [2] and tags[322][2] == tags[323][2] == [16]
        assert tags[324][0] == tags[325][0] == (16 if big else 4)
        assert tags[324][2] == offsets[k] and tags[325][2] == counts[k] and len(counts[k]) == 3 * -(-lay.H // 16) * -(-lay.W // 16)
        assert all(b == a + c for a, b, c in zip(offsets[k], offsets[k][1:], counts[k])), "a level's segments lie back to back"
        spans.append((offsets[k][0], offsets[k][0] + bodies[k]))
        geo_here = {t: v for t, v in tags.items() if t >= 33550}
        assert (set(geo_here) == {g[0] for g in H.GEO}) if (k == 0 and geo) else not geo_here
        if k == 0 and geo:
            assert [(t, geo_here[t][0], geo_here[t][1], geo_here[t][2] if isinstance(geo_here[t][2], bytes) else
                     struct.pack("<%dH" % geo_here[t][1], *geo_here[t][2])) for t in sorted(geo_here)] == H.GEO
    # smallest level first, the full resolution last, nothing overlaps, everything inside the file
    order = sorted(range(nlevels + 1), key=lambda k: spans[k][0])
    assert order == list(range(nlevels, -1, -1))
    for a, b in zip(order, order[1:]):
        assert spans[a][1] == spans[b][0]
    total = len(head) + sum(bodies)
    assert spans[0][1] == total and all(o + c <= total for k in range(nlevels + 1) for o, c in zip(offsets[k], counts[k]))
    if fake == (1 << 32) - 20000:
        assert total <= 0xFFFFFFFF
    # the decision is made on the end of the last segment
    if fake is None:
        classic_head = len(head)
        at_limit = 0xFFFFFFFF - classic_head - sum(bodies[1:])
        for body0, want_big in ((at_limit, False), (at_limit + 1, True)):
            h2, _ = tiff_write.assemble_pyramid(lays, counts, geo, body_bytes=[body0] + bodies[1:])
            assert (struct.unpack_from("<H", h2, 2)[0] == 43) == want_big
        assert walk(tiff_write.assemble_pyramid(lays, counts, geo, force_big=True)[0])[1]


def test_one_level_and_no_geo_is_assemble_byte_for_byte():
    from lbdrn_hip import tiff_write
    for lay in (_layouts(3, 75, 130, 16, 0)[0], _layouts(3, 40, 50, 8, 0, planar=1)[0],
                tiff_write.make_layout(2, 37, 53, 16, "none", None, 8, 2, None, cap=1 << 20)):
        counts = list(range(5, 5 + tiff_write.segment_count(lay)))
        for kw in (dict(), dict(force_big=True), dict(sample_format=1)):
            head, offsets = tiff_write.assemble(lay, counts, **kw)
            for geo in (None, [], ()):
                h2, o2 = tiff_write.assemble_pyramid([lay], [counts], geo, **kw)
                assert h2 == head and o2 == [offsets]
        head, offsets = tiff_write.assemble(lay, counts, body_bytes=1 << 32)
        assert tiff_write.assemble_pyramid([lay], [counts], body_bytes=[1 << 32]) == (head, [offsets])
        # with geo, the file differs by those tags alone: the same tags otherwise, the same data order
        if lay.tiled:
            head, _ = tiff_write.assemble(lay, counts)
            h3, o3 = tiff_write.assemble_pyramid([lay], [counts], H.GEO)
            (_, tags, _), = walk(h3)[0]
            (_, plain, _), = walk(head)[0]
            assert {t: v for t, v in tags.items() if t < 33550 and t not in (324,)} == {t: v for t, v in plain.items() if t != 324}
            assert len(h3) > len(head) and o3[0][0] == len(h3)


# ---------------------------------------------------------------- whole files

def _frames(path):
    from PIL import Image
    out = []
    with Image.open(path) as im:
        for k in range(im.n_frames):
            im.seek(k)
            out.append(np.asarray(im).copy())
    return out


@pytest.mark.parametrize("case", ("one 16-bit band", "three chunky 8-bit bands"))
def test_whole_files_read_by_pillow_and_by_the_package_parser(shim, tiffw_shim, tmp_path, case):
    from lbdrn_hip import tiff
    if case == "one 16-bit band":
        a, planar = TW.base_raster(C=1, H=75, W=130), 2
    else:
        a, planar = TW.base_raster(C=3, H=75, W=130, dtype=np.uint8), 1
    for resampling, nodata in (("average", None), ("average", 513), ("nearest", None)):
        nodata = nodata if a.dtype == np.uint16 or nodata is None else 1
        buf, lays, offsets, counts = H.host_write(shim, tiffw_shim, a, 16, "auto", resampling, nodata, H.GEO, planar)
        want = [a] + R.pyramid(a, 4, resampling, nodata)
        assert [(lay.H, lay.W) for lay in lays] == [w.shape[1:] for w in want] == [(75, 130), (38, 65), (19, 33), (10, 17), (5, 9)]
        # the package's parser and the reference decoders
        assert len(tiff.read_ifds(buf)) == 5 and tiff.overview_ifds(buf) == [1, 2, 3, 4]
        for k in range(5):
            sc = tiff.parse(buf, "p.tif", ifd=k)
            assert sc.shape == want[k].shape and sc.layout.seg_w == sc.layout.seg_h == 16 and sc.layout.planar == planar
            assert sc.offsets.tolist() == offsets[k] and sc.counts.tolist() == list(counts[k])
            got = _read_level(buf, k)
            assert np.array_equal(got, want[k]), (case, resampling, nodata, k)
        with pytest.raises(IndexError, match="has 5"):
            tiff.parse(buf, "p.tif", ifd=5)
        assert tiff.read_geo_tags(buf) == H.GEO
        # Pillow
        path = str(tmp_path / "p.tif")
        with open(path, "wb") as f:
            f.write(buf)
        try:
            frames = _frames(path)
        except ImportError as e:
            pytest.skip(f"Pillow does not import: {e}")
        except Exception as e:      # noqa: BLE001
            if "decoder" in str(e) and "not available" in str(e):
                pytest.skip(f"this Pillow has no libtiff: {e}")
            raise
        assert len(frames) == 5
        for k, fr in enumerate(frames):
            assert np.array_equal(fr, want[k][0] if a.shape[0] == 1 else want[k].transpose(1, 2, 0)), (case, resampling, nodata, k)
    # without overviews and geo: the file of write_segments
    buf, lays, _, counts = H.host_write(shim, tiffw_shim, a, 16, None, planar=planar)
    body = TW.host_encode(tiffw_shim, a, lays[0])[0].tobytes()
    from lbdrn_hip import tiff_write
    assert buf == tiff_write.assemble(lays[0], counts[0])[0] + body and len(tiff.read_ifds(buf)) == 1


def _read_level(buf, k):
    """tests/tiff_write_helpers.reference_read for IFD k"""
    from lbdrn_hip import tiff
    sc = tiff.parse(buf, ifd=k)
    lay = sc.layout
    spp = 1 if lay.planar == 2 else lay.C
    segs = [TW.R.decompress(bytes(buf[o:o + n]), lay.compression, lay.seg_h * lay.seg_w * spp * lay.bits // 8)
            for o, n in zip(sc.offsets.tolist(), sc.counts.tolist())]
    return TW.R.place_segments(segs, lay.C, lay.H, lay.W, np.uint8 if lay.bits == 8 else np.uint16, tile=(lay.seg_w, lay.seg_h),
                               rows_per_strip=lay.seg_h, planar=lay.planar, predictor=lay.predictor, byteorder="<")


def test_a_looped_chain_and_one_that_leaves_the_file_are_refused(shim, tiffw_shim):
    from lbdrn_hip import tiff
    a = TW.base_raster(C=1, H=37, W=53)
    buf = H.host_write(shim, tiffw_shim, a, 16, 2)[0]
    ifds = tiff.read_ifds(buf)
    assert len(ifds) == 3 and ifds[0] == 8
    ends = [walk(buf)[0][k][0] + 2 + 12 * len(walk(buf)[0][k][1]) for k in range(3)]      # where each next-IFD field lies
    assert struct.unpack_from("<I", buf, ends[0])[0] == ifds[1] and struct.unpack_from("<I", buf, ends[2])[0] == 0
    for target in (ifds[0], ifds[1], ifds[2]):
        bad = bytearray(buf)
        struct.pack_into("<I", bad, ends[2], target)
        with pytest.raises(ValueError, match="loops"):
            tiff.read_ifds(bytes(bad))
        with pytest.raises(ValueError, match="loops"):
            tiff.parse(bytes(bad), ifd=1)
        assert tiff.parse(bytes(bad)).shape == a.shape      # the first IFD alone is read as it always was
    for target in (len(buf), len(buf) - 1, len(buf) + 4096, 0xFFFFFFF0):
        bad = bytearray(buf)
        struct.pack_into("<I", bad, ends[1], target)
        with pytest.raises(ValueError, match="outside the file"):
            tiff.read_ifds(bytes(bad))
        with pytest.raises(ValueError, match="outside the file"):
            tiff.overview_ifds(bytes(bad))
    # an entry count that runs over the end
    bad = bytearray(buf)
    struct.pack_into("<H", bad, ifds[2], 60000)
    with pytest.raises(ValueError, match="outside the file"):
        tiff.read_ifds(bytes(bad))
    # a second IFD that is no overview (a page) is not a level
    bad = bytearray(buf)
    (_, tags, _) = walk(buf)[0][1]
    at = ifds[1] + 2 + 12 * sorted(tags).index(254) + 8
    struct.pack_into("<I", bad, at, 2)
    assert tiff.overview_ifds(bytes(bad)) == [2]


# ---------------------------------------------------------------- georeferencing tags

@pytest.mark.parametrize("which", range(len(H.GEO)), ids=[str(g[0]) for g in H.GEO])
def test_each_geo_tag_comes_back_as_given(shim, tiffw_shim, which):
    from lbdrn_hip import tiff
    a = TW.base_raster(C=2, H=37, W=53)
    geo = [H.GEO[which]]
    for overviews in (None, "auto"):
        buf = H.host_write(shim, tiffw_shim, a, 16, overviews, geo=geo)[0]
        assert tiff.read_geo_tags(buf) == geo
        ifds, _ = walk(buf)
        assert len(ifds) == (1 if overviews is None else 3)
        for k, (_, tags, _) in enumerate(ifds):
            assert (geo[0][0] in tags) == (k == 0)
            assert not any(t >= 33550 for t in tags if t != geo[0][0])
        assert np.array_equal(_read_level(buf, 0), a)


def test_geo_tags_of_other_files_either_byte_order_and_none(shim, tiffw_shim, tmp_path):
    from lbdrn_hip import raster_io, tiff
    a = TW.base_raster(C=2, H=20, W=31)
    for bo in ("<", ">"):
        plain = TW.R.write_tiff(a, byteorder=bo, rows_per_strip=1, compression=TW.R.COMP_LZW, predictor=2)[0]
        assert tiff.read_geo_tags(plain) == []
        tagged = H.with_tags(plain, H.GEO)
        assert tiff.read_geo_tags(tagged) == H.GEO
        assert tiff.parse(tagged).shape == a.shape and tiff.parse(tagged).offsets.tolist() == tiff.parse(plain).offsets.tolist()
        path = str(tmp_path / f"t{ord(bo)}.tif")
        with open(path, "wb") as f:
            f.write(tagged)
        assert raster_io.read_geo_tags(path) == H.GEO
    # the package's own uncompressed writer and the GPU writer's plain files carry none
    path = str(tmp_path / "plain.tif")
    raster_io._write_tiff(path, a)
    assert raster_io.read_geo_tags(path) == []
    assert tiff.read_geo_tags(H.host_write(shim, tiffw_shim, a, 16, "auto")[0]) == []
    # a tag of another type than its own is not taken
    odd = H.with_tags(TW.R.write_tiff(a)[0], [(34735, 3, 4, b"\1\0\1\0\0\0\0\0")])
    assert tiff.read_geo_tags(odd) == [(34735, 3, 4, b"\1\0\1\0\0\0\0\0")]
    at = odd.rindex(struct.pack("<HH", 34735, 3))
    assert tiff.read_geo_tags(odd[:at + 2] + struct.pack("<H", 4) + odd[at + 4:]) == []
    with pytest.raises(ValueError, match="outside the file"):
        tiff.read_geo_tags(odd[:-3])


# ---------------------------------------------------------------- the command lines' refusals

def test_decode_refuses_the_overview_flags_without_their_partner(capsys, tmp_path):
    import decode
    for argv, word in ((["--out-overviews", "auto"], "--out-compress"), (["--out-resampling", "nearest"], "--out-compress"),
                       (["--out-nodata", "0"], "--out-compress"), (["--out-georef", "x.tif"], "--out-compress"),
                       (["--out-compress", "deflate", "--out-resampling", "nearest"], "--out-overviews"),
                       (["--out-compress", "deflate", "--out-nodata", "0"], "--out-overviews"),
                       (["--out-compress", "deflate", "--out-overviews", "some"], "auto or a count"),
                       (["--out-compress", "deflate", "--out-overviews", "-1"], "auto or a count"),
                       (["--out-compress", "deflate", "--out-overviews", "2", "--out-resampling", "cubic"], "invalid choice"),
                       (["--out-compress", "deflate", "--out-overviews", "2", "--out-nodata", "70000"], "sample value"),
                       (["--out-compress", "deflate", "--out-georef", str(tmp_path / "missing.tif")], "no such file")):
        with pytest.raises(SystemExit) as e:
            decode.main(["-i", "x.bin"] + argv, shard_tiles=False)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_module_command_line_refuses_bad_arguments(capsys):
    from lbdrn_hip import pyramid
    for argv, word in ((["a.tif"], "required"), (["a.tif", "b.tif", "--overviews", "some"], "overviews"),
                       (["a.tif", "b.tif", "--overviews", "-2"], "overviews"), (["a.tif", "b.tif", "--resampling", "cubic"], "invalid choice"),
                       (["a.tif", "b.tif", "--nodata", "-1"], "sample value"), (["a.tif", "b.tif", "--nodata", "x"], "invalid int"),
                       (["a.tif", "b.tif", "--tile", "20"], "multiple of 16"), (["a.tif", "b.npy"], "TIFF"), (["a.npy", "b.tif"], "TIFF")):
        with pytest.raises(SystemExit) as e:
            pyramid.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


# ---------------------------------------------------------------- the kernels' resources

def test_no_kernel_of_the_library_has_scratch_or_spilled_registers():
    from lbdrn_hip import pyramid
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    if not os.path.exists(os.path.join(KR.LLVM, "llvm-objdump")) or not os.path.exists(pyramid._PATH):
        pytest.skip("llvm-objdump or the library is missing")
    rows = [r for r in KR.kernel_resources(pyramid._PATH) if "k_pyr_" in r["demangled"]]
    assert len(rows) == 6 and all("k_pyr_reduce" in r["demangled"] for r in rows)      # 8 / 16 bits x average, average with nodata, nearest
    for r in rows:
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["spill_sgpr"] == 0 and r["lds"] == 0, r
        assert r["vgpr"] + r["agpr"] <= 64, r      # eight waves a SIMD


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_the_host_build_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "pyramid_main")
    cmd = [TW.cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "pyramid_main.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "486 builds, 0 failed" in run.stdout and "ERROR" not in run.stderr
