"""The TIFF writer on the CPU: lbdrn_hip/tiff_write.py's container around segments made by the host build of csrc/tiffw.inc
(tests/tiff_write_host_shim.cpp, g++: the text the device runs, its 64 lanes a loop), judged by three readers -- zlib,
the project's own parser and reference decoders (lbdrn_hip.tiff.parse, tests/tiff_reference.py), and Pillow where it
imports; the length-limited code lengths on chosen histograms; the encoder's hard segments; its size against zlib on the
golden rasters; raster_io.write_raster end to end with the device stage replaced by the host build; the library's checks
that come before any launch; the kernels' resource usage; and tests/tiff_write_main.cpp, a stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU.  Every comparison of sample values is exact."""
import ctypes
import heapq
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_write_helpers as H  # noqa: E402
from tiff_write_helpers import CSRC, ROOT  # noqa: E402

R = H.R


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return H.load_shim(tmp_path_factory)


def _layout(a, seg, planar, compress, predictor):
    from lbdrn_hip import tiff_write
    return tiff_write.make_layout(a.shape[0], a.shape[1], a.shape[2], a.dtype.itemsize * 8, compress, planar=planar, predictor=predictor,
                                  cap=1 << 20, **seg)


# ---------------------------------------------------------------- the container

@pytest.mark.parametrize("big", (False, True), ids=("classic", "bigtiff"))
def test_container_parses_and_decodes_on_every_layout(shim, big):
    from lbdrn_hip import tiff, tiff_write
    n = 0
    for dtype in (np.uint8, np.uint16):
        full = H.base_raster(dtype=dtype)
        for bands in (1, 3, 4, 8):
            a = np.ascontiguousarray(full[:bands])
            for seg in H.SEGMENTATIONS:
                for planar in (1, 2):
                    for compress, pred in H.CODINGS:
                        lay = _layout(a, seg, planar, compress, pred)
                        body, offsets, counts = H.host_encode(shim, a, lay)
                        head, file_offsets = tiff_write.assemble(lay, counts, force_big=big)
                        buf = head + body.tobytes()
                        assert buf[2] == (43 if big else 42)
                        sc = tiff.parse(buf)
                        for name, _ in tiff.Layout._fields_:
                            assert getattr(sc.layout, name) == getattr(lay, name), (name, seg, planar, compress, pred)
                        assert sc.offsets.tolist() == file_offsets == (offsets + np.uint64(len(head))).tolist()
                        assert sc.counts.tolist() == counts.tolist()
                        got = H.reference_read(buf)
                        assert got.dtype == a.dtype and np.array_equal(got, a), (seg, planar, compress, pred, bands, dtype)
                        if compress == "deflate":      # zlib on every segment: the gathered bytes, the reference's own
                            want = R.raw_segments(a, tile=seg.get("tile"), rows_per_strip=seg.get("rows_per_strip"), planar=planar,
                                                  predictor=pred)
                            for o, c, w in zip(file_offsets, counts.tolist(), want):
                                assert zlib.decompress(buf[o:o + c]) == w
                        n += 1
    assert n == 2 * 4 * 5 * 2 * 3


def test_the_tags_are_those_of_write_tiff_plus_the_new_ones(shim, tmp_path):
    from lbdrn_hip import raster_io, tiff, tiff_write
    a = H.base_raster()[:3]
    plain = str(tmp_path / "plain.tif")
    raster_io._write_tiff(plain, a)

    def tags(buf):
        n = struct.unpack_from("<H", buf, 8)[0]
        return [struct.unpack_from("<H", buf, 10 + 12 * i)[0] for i in range(n)]
    old = tags(open(plain, "rb").read())
    lay = _layout(a, dict(tile=(16, 16)), 2, "deflate", 2)
    head, _ = tiff_write.assemble(lay, H.host_encode(shim, a, lay)[2])
    new = tags(head)
    assert new == sorted(new)
    assert set(new) == (set(old) - {273, 278, 279}) | {317, 322, 323, 324, 325}
    lay = _layout(a, dict(rows_per_strip=8), 1, "deflate", 1)
    head, _ = tiff_write.assemble(lay, H.host_encode(shim, a, lay)[2])
    assert set(tags(head)) == set(old)      # strips, no predictor: the same tags, other values
    assert tiff.read_tags(head + b"\0" * 8)[0][259] == [8]


def test_bigtiff_is_chosen_where_an_offset_would_pass_32_bits():
    from lbdrn_hip import tiff_write
    lay = tiff_write.Layout(4, 4096, 4096, 16, 0, 2, 256, 256, 1, 8, 2)
    counts = [1000] * 1024
    head, offsets = tiff_write.assemble(lay, counts)
    assert head[2] == 42 and offsets[0] == len(head)
    fits = 0xFFFFFFFF - len(head)      # the body that ends exactly at the last classic offset
    assert tiff_write.assemble(lay, counts, body_bytes=fits)[0] == head
    big, boffsets = tiff_write.assemble(lay, counts, body_bytes=fits + 1)
    assert big[2] == 43 and struct.unpack_from("<HHQ", big, 4) == (8, 0, 16) and boffsets[0] == len(big)
    # LONG8 tables in it: offsets that classic TIFF cannot hold survive
    counts = [3 << 30, 3 << 30, 5]
    lay = tiff_write.Layout(3, 16, 16, 8, 0, 2, 16, 16, 1, 8, 1)
    big, boffsets = tiff_write.assemble(lay, counts)
    assert big[2] == 43 and boffsets[2] == len(big) + (6 << 30)
    from lbdrn_hip import tiff
    tags = tiff.read_tags(big)[0]
    assert tags[324] == boffsets and tags[325] == counts


# ---------------------------------------------------------------- code lengths

def _huffman_cost(freq):
    """the cost in bits of a minimum-redundancy code, and its greatest depth over all optimal trees built by the heap"""
    heap = [(f, 0) for f in freq if f]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (f1, d1), (f2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        cost += f1 + f2
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1))
    return cost, heap[0][1]


def _lengths(shim, freq, limit):
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.full(len(f) + 8, 0x77, np.uint8)
    shim.tiffw_shim_lengths(f.ctypes.data, len(f), limit, out.ctypes.data)
    assert (out[len(f):] == 0x77).all()
    return out[:len(f)].astype(int)


def _check_lengths(shim, freq, limit):
    freq = np.asarray(freq)
    ln = _lengths(shim, freq, limit)
    used = int((freq > 0).sum())
    assert ((ln > 0) == (freq > 0)).all()
    assert ln.max() <= limit
    kraft = sum(2 ** (limit - l) for l in ln if l)
    assert kraft <= 2 ** limit and (kraft == 2 ** limit or used < 2), (kraft, used)
    cost, depth = _huffman_cost(freq.tolist())
    got = int((ln * freq).sum())
    if depth <= limit:      # an unrestricted Huffman code fits: the lengths are one (code lengths are unique up to ties: by cost)
        assert got == cost, (got, cost)
    else:
        assert got >= cost
    # a more frequent symbol never has the longer code
    order = np.argsort(freq[freq > 0], kind="stable")
    assert (np.diff(ln[freq > 0][order]) <= 0).all()
    return ln


def test_code_lengths_are_limited_complete_and_optimal_where_that_fits(shim):
    rng = np.random.default_rng(23)
    for k in range(60):
        n = (286, 30, 19)[k % 3]
        limit = 7 if n == 19 else 15
        freq = rng.integers(0, (2, 50, 5000)[k % 3 - 1] + 1, n) * (rng.random(n) < rng.random())
        if freq.sum():
            _check_lengths(shim, freq, limit)
    skew = (rng.pareto(0.4, 286) * 3).astype(np.uint64).clip(0, 2 ** 24)      # heavy tails: deep unrestricted trees
    _check_lengths(shim, skew, 15)
    one = np.zeros(286, int)
    one[256] = 9
    assert _check_lengths(shim, one, 15)[256] == 1
    two = one.copy()
    two[7] = 1000
    assert _check_lengths(shim, two, 15)[[7, 256]].tolist() == [1, 1]
    assert sorted(_check_lengths(shim, np.full(286, 5), 15).tolist()) == [8] * 226 + [9] * 60
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert _huffman_cost(fib)[1] == 23
    f = np.zeros(286, int)
    f[10:34] = fib
    assert _check_lengths(shim, f, 15).max() == 15      # depth 23 without the limit
    f = np.zeros(19, int)
    f[:19] = fib[:19]
    assert _huffman_cost(f.tolist())[1] == 18 and _check_lengths(shim, f, 7).max() == 7
    assert _check_lengths(shim, np.arange(1, 20), 7).max() <= 7


def test_code_length_stream_runs(shim):
    """16 / 17 / 18: zero runs of 138 and 139, of 10 and 11, of 2 and 3, and repeats of 6, 7 and 9 of a length"""
    def rle(ll, d):
        ll, d = np.asarray(ll, np.uint8), np.asarray(d, np.uint8)
        out = np.zeros(len(ll) + len(d) + 4, np.uint16)
        n = shim.tiffw_shim_rle(ll.ctypes.data, len(ll), d.ctypes.data, len(d), out.ctypes.data)
        assert n <= len(ll) + len(d)
        return [(int(v) & 255, int(v) >> 8) for v in out[:n]]

    def expand(syms):
        out = []
        for s, e in syms:
            if s < 16:
                out.append(s)
            elif s == 16:
                assert 0 <= e <= 3 and out
                out += [out[-1]] * (3 + e)
            elif s == 17:
                assert 0 <= e <= 7
                out += [0] * (3 + e)
            else:
                assert s == 18 and 0 <= e <= 127
                out += [0] * (11 + e)
        return out
    for gap, want in ((138, [(18, 127)]), (139, [(18, 127), (0, 0)]), (10, [(17, 7)]), (11, [(18, 0)]), (2, [(0, 0), (0, 0)]), (3, [(17, 0)]),
                      (149, [(18, 127), (18, 0)]), (276, [(18, 127), (18, 127)])):
        ll = [5] + [0] * gap + [6] * (285 - gap)
        syms = rle(ll[:286], [3])
        assert syms[:1 + len(want)] == [(5, 0)] + want, (gap, syms[:4])
        assert expand(syms) == ll[:286] + [3]
    for rep, want in ((7, [(9, 0), (16, 3)]), (8, [(9, 0), (16, 3), (9, 0)]), (10, [(9, 0), (16, 3), (16, 0)]), (3, [(9, 0), (9, 0), (9, 0)])):
        ll = [9] * rep + [0] * (257 - rep)
        syms = rle(ll, [0])
        assert syms[:len(want)] == want and expand(syms) == ll + [0]
    # a run goes on from the literal/length lengths into the distance lengths, as RFC 1951 allows
    assert rle([0] * 256 + [4, 4], [4, 4, 4])[-2:] == [(4, 0), (16, 1)]


# ---------------------------------------------------------------- whole segments

def _blocks(stream):
    """(BFINAL, BTYPE) of the first block and, for a dynamic one, HLIT, HDIST, HCLEN as counts"""
    v = int.from_bytes(stream[2:6], "little")
    return v & 1, (v >> 1) & 3, 257 + ((v >> 3) & 31), 1 + ((v >> 8) & 31), 4 + ((v >> 13) & 15)


def test_hard_segments_inflate_to_their_input(shim):
    cap = shim.tiffw_shim_block_tokens()
    seen = 0
    for name, data in H.special_segments(cap).items():
        z, st = H.shim_deflate(shim, data)
        assert zlib.decompress(z) == data, name
        assert H.shim_deflate(shim, data, 0x00)[0] == z == H.shim_deflate(shim, data, 0xFF)[0], name      # whatever the state held
        assert z[:2] == b"\x78\x01" and z[-4:] == struct.pack(">I", zlib.adler32(data)), name
        final, kind, hlit, hdist, _ = _blocks(z)
        seen |= st[2]
        if name == "constant 128 KiB":      # 258-byte matches at distance 1
            assert st[0] == 1 and st[1] <= 3 + (131072 + 257) // 258 and len(z) < 200
        elif name == "32 KiB of noise three times":
            assert len(z) < 98304      # the second and third copy lie exactly 32768 bytes behind: some of it is found
        elif name == "128 KiB of noise":
            assert st[2] == 1 and st[3] > st[0] - 1 >= 2 and len(z) > 131072      # stored, several blocks, inside the bound
        elif name == "one token more than a block":
            assert st[:2] == [2, cap + 1] and final == 0
            assert zlib.decompressobj().decompress(z) == data
        elif name == "literals only":
            assert st[:3] == [1, len(data), 4] and (final, kind, hdist) == (1, 2, 1)      # one distance length, and it is zero
        elif name == "one distance":
            assert st[2] == 4 and kind == 2 and len(z) < 100
        elif name.startswith("zero run"):
            assert st[2] == 4 and kind == 2
    assert seen == 7      # stored, fixed and dynamic blocks were all written
    # a stored segment above 65535 bytes in one block cannot happen (a block holds at most block_tokens literals); a block of
    # long matches that is cheapest stored cannot either.  Both splits are still written correctly: see lbdrn_tiffw_bound.
    noise = H.special_segments(cap)["128 KiB of noise"]
    assert len(H.shim_deflate(shim, noise)[0]) <= shim.tiffw_shim_bound(len(noise))
    assert shim.tiffw_shim_adler32(b"\xff" * 70000, 70000) == zlib.adler32(b"\xff" * 70000)


def test_size_against_zlib_on_the_golden_rasters(shim, capsys):
    """total segment bytes below Huffman-only zlib (matches are found and used), and within 0.02 of the recorded ratio to
    zlib level 1 (the bytes are deterministic: the margin only absorbs later deliberate changes)"""
    from lbdrn_hip import tiff_write
    for name, tile, recorded in H.GOLDEN_SETUPS:
        img = H.golden_planes(name)
        lay = tiff_write.make_layout(*img.shape, 16, "deflate", tile=tile, planar=2, predictor=2, cap=1 << 20)
        stage = {}
        H.host_encode(shim, img, lay, stage)
        ours = sum(len(c) for c in stage["coded"])
        huff = sum(len(H.huffman_only(r)) for r in stage["raw"])
        z1 = sum(len(zlib.compress(r, 1)) for r in stage["raw"])
        raw = sum(len(r) for r in stage["raw"])
        with capsys.disabled():
            print(f"\n{name}: writer {ours / raw:.4f} of raw, Huffman-only {huff / raw:.4f}, zlib -1 {z1 / raw:.4f}, writer / zlib -1 = {ours / z1:.4f}")
        assert ours < huff
        assert ours / z1 <= recorded + 0.02
        for r, c in zip(stage["raw"], stage["coded"]):
            assert zlib.decompress(c) == r


# ---------------------------------------------------------------- raster_io.write_raster

def _host_write(shim):
    from lbdrn_hip import tiff_write

    def write(path, array, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None, device=None):
        a = np.ascontiguousarray(array if array.ndim == 3 else array[None])
        lay = tiff_write.make_layout(a.shape[0], a.shape[1], a.shape[2], a.dtype.itemsize * 8, compress, tile, rows_per_strip, planar,
                                     predictor, cap=shim.tiffw_shim_cap(8 if compress == "deflate" else 1))
        body, _, counts = H.host_encode(shim, a, lay)
        tiff_write.write_segments(path, lay, body, counts)
        return lay
    return write


def test_write_raster_defaults_write_what_they_always_wrote(tmp_path):
    from lbdrn_hip import raster_io
    if raster_io._gdal() is not None:
        pytest.skip("GDAL writes the file here")
    for dtype in (np.uint8, np.uint16, np.float32):
        a = H.base_raster(C=3, dtype=np.uint16).astype(dtype)
        one, two, three = (str(tmp_path / f"{k}.tif") for k in "abc")
        raster_io.write_raster(one, a)
        raster_io._write_tiff(two, a)
        raster_io.write_raster(three, a, compress=None, tile=None, rows_per_strip=None, planar=2, predictor=None)
        assert open(one, "rb").read() == open(two, "rb").read() == open(three, "rb").read()


def test_write_raster_end_to_end_with_the_device_stage_on_the_host(shim, tmp_path, monkeypatch):
    from lbdrn_hip import raster_io, tiff, tiff_write
    if raster_io._gdal() is not None:
        pytest.skip("GDAL reads the file first here")
    monkeypatch.setattr(tiff_write, "write", _host_write(shim))

    def host_read(path, device=None):
        a = H.reference_read(open(path, "rb").read())
        return a[0] if a.shape[0] == 1 else a
    monkeypatch.setattr(tiff, "read", host_read)
    path = str(tmp_path / "t.tif")
    for bands, dtype in ((4, np.uint16), (1, np.uint16), (3, np.uint8)):
        a = H.base_raster(C=bands, H=300, W=270, dtype=dtype)
        for kw, want in ((dict(compress="deflate"), (1, 256, 256, 8, 2, 2)), (dict(tile=32), (1, 32, 32, 1, 1, 2)),
                         (dict(compress="deflate", rows_per_strip=64, planar=1, predictor=1), (0, 270, 64, 8, 1, 1)),
                         (dict(compress="deflate", tile=(64, 16)), (1, 64, 16, 8, 2, 2))):
            raster_io.write_raster(path, a, **kw)
            lay = tiff.parse(open(path, "rb").read()).layout
            assert (lay.tiled, lay.seg_w, lay.seg_h, lay.compression, lay.predictor, lay.planar) == want
            got = raster_io.read_raster(path)
            assert got.dtype == a.dtype and np.array_equal(got.reshape(a.shape), a) and got.ndim == (3 if bands > 1 else 2)
    smooth = H.golden_planes("rasters_learn_bands4.npz")
    raster_io.write_raster(path, smooth, compress="deflate")
    assert os.path.getsize(path) < 0.45 * smooth.nbytes


def test_value_errors(shim, tmp_path):
    from lbdrn_hip import raster_io, tiff_write
    a = H.base_raster(C=2)
    path = str(tmp_path / "t.tif")
    for side in (17, 8, 250, 0, -16):
        with pytest.raises(ValueError, match=rf"tile side {side}\b.*multiple of 16"):
            raster_io.write_raster(path, a, compress="deflate", tile=side)
    with pytest.raises(ValueError, match=r"tile side 24\b"):
        raster_io.write_raster(path, a, tile=(32, 24))
    cap = tiff_write.lib().lbdrn_tiffw_segment_cap(8)
    assert cap == shim.tiffw_shim_cap(8)
    with pytest.raises(ValueError, match=rf"above the cap of {cap} bytes"):
        raster_io.write_raster(path, np.zeros((1, 1024, 1024), np.uint16), compress="deflate", tile=1024)
    with pytest.raises(ValueError, match=rf"above the cap of {cap} bytes"):
        raster_io.write_raster(path, np.zeros((3, 300, 2048), np.uint16), compress="deflate", rows_per_strip=300, planar=1)
    for dtype in (np.float32, np.float64):
        with pytest.raises(ValueError, match="written uncompressed only"):
            raster_io.write_raster(path, a.astype(dtype), compress="deflate")
        with pytest.raises(ValueError, match="written uncompressed only"):
            raster_io.write_raster(path, a.astype(dtype), tile=16)
    with pytest.raises(ValueError, match="compress = 'lzw'"):
        raster_io.write_raster(path, a, compress="lzw")
    with pytest.raises(ValueError, match="exclude each other"):
        raster_io.write_raster(path, a, compress="deflate", tile=16, rows_per_strip=4)
    with pytest.raises(ValueError, match="predictor 2 goes with Deflate"):
        raster_io.write_raster(path, a, tile=16, predictor=2)
    with pytest.raises(ValueError, match="not of a .npy"):
        raster_io.write_raster(str(tmp_path / "t.npy"), a, compress="deflate")
    assert not os.path.exists(path)


def test_without_a_device_the_writer_raises_the_no_cpu_path_error(tmp_path):
    import torch
    from lbdrn_hip import raster_io, tiff_write
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(tiff_write.TiffWriteError, match="no CPU path"):
        raster_io.write_raster(str(tmp_path / "t.tif"), H.base_raster(C=2), compress="deflate")


# ---------------------------------------------------------------- the library's checks that come before any launch

def test_library_refuses_before_any_launch(shim):
    from lbdrn_hip import tiff, tiff_write
    L = tiff_write.lib()
    lay = tiff_write.Layout(8, 37, 53, 16, 0, 2, 53, 1, 0, 8, 2)
    assert L.lbdrn_tiffw_abi_version() == 1
    assert L.lbdrn_tiffw_segment_count(ctypes.byref(lay)) == 296
    assert L.lbdrn_tiffw_block_tokens() == shim.tiffw_shim_block_tokens()
    assert [L.lbdrn_tiffw_segment_cap(c) > 0 for c in (1, 8, 5, 32773, 7, 32946)] == [True] * 2 + [False] * 4
    assert L.lbdrn_tiffw_segment_cap(8) <= tiff.lib().lbdrn_tiff_segment_cap(8)      # what is written the device reader reads
    for n in (1, 106, 4096, 65535, 65536, 131072, 786432):
        assert L.lbdrn_tiffw_bound(n) == shim.tiffw_shim_bound(n) and n + 6 < L.lbdrn_tiffw_bound(n) <= n + n // 300 + 64
    assert L.lbdrn_tiffw_output_bytes(ctypes.byref(lay)) == 296 * L.lbdrn_tiffw_bound(106)
    assert L.lbdrn_tiffw_workspace(ctypes.byref(lay)) >= 296 * (112 + L.lbdrn_tiffw_bound(106))
    for field, value in (("C", 0), ("bits", 12), ("planar", 3), ("seg_w", 52), ("seg_h", 38), ("compression", 5), ("compression", 32773),
                         ("predictor", 3), ("W", (1 << 20) + 1), ("big_endian", 1)):
        bad = tiff_write.Layout(*[getattr(lay, n) for n, _ in tiff_write.Layout._fields_])
        setattr(bad, field, value)
        assert L.lbdrn_tiffw_segment_count(ctypes.byref(bad)) == 0 and L.lbdrn_tiffw_workspace(ctypes.byref(bad)) == 0 and \
            L.lbdrn_tiffw_output_bytes(ctypes.byref(bad)) == 0, field
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before any device work
    nws, nout = L.lbdrn_tiffw_workspace(ctypes.byref(lay)), L.lbdrn_tiffw_output_bytes(ctypes.byref(lay))

    def call(lay, out_bytes, ws_bytes, planes=fake):
        return L.lbdrn_tiffw_encode(ctypes.byref(lay), planes, fake, out_bytes, fake, fake, fake, fake, ws_bytes, None)
    assert call(lay, nout, nws, None) == tiff_write.E_ARG and b"null" in L.lbdrn_tiffw_last_error()
    assert call(bad, nout, nws) == tiff_write.E_ARG and b"out of range" in L.lbdrn_tiffw_last_error()
    assert call(lay, nout - 1, nws) == tiff_write.E_ARG and b"out holds" in L.lbdrn_tiffw_last_error()
    assert call(lay, nout, nws - 1) == tiff_write.E_WORKSPACE and b"workspace" in L.lbdrn_tiffw_last_error()
    assert call(lay, nout, 0) == tiff_write.E_WORKSPACE
    big = tiff_write.Layout(1, 2048, 2048, 16, 0, 2, 1024, 1024, 1, 8, 2)      # tiles of 2 MiB
    bout = L.lbdrn_tiffw_output_bytes(ctypes.byref(big))
    # precedence: E_ARG, then E_UNSUPPORTED, then E_WORKSPACE
    assert call(big, bout, 0) == tiff_write.E_UNSUPPORTED and b"cap" in L.lbdrn_tiffw_last_error()
    assert call(big, bout - 1, 0) == tiff_write.E_ARG


def test_no_kernel_of_the_library_has_scratch_or_spilled_registers():
    from lbdrn_hip import tiff_write
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    if not os.path.exists(os.path.join(KR.LLVM, "llvm-objdump")) or not os.path.exists(tiff_write._PATH):
        pytest.skip("llvm-objdump or the library is missing")
    rows = [r for r in KR.kernel_resources(tiff_write._PATH) if "k_tiffw_" in r["demangled"]]
    names = " ".join(r["demangled"] for r in rows)
    assert all(k in names for k in ("k_tiffw_gather", "k_tiffw_deflate", "k_tiffw_pack")) and len(rows) == 4
    for r in rows:
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 160 * 1024, r


# ---------------------------------------------------------------- Pillow (libtiff) as the third reader

def test_pillow_reads_the_two_shapes_it_knows(shim, tmp_path):
    try:
        from PIL import Image
    except Exception as e:      # noqa: BLE001
        pytest.skip(f"Pillow does not import: {e}")
    from lbdrn_hip import tiff_write
    path = str(tmp_path / "p.tif")
    for a, planar in ((H.base_raster(C=1, H=150, W=203), 2), (H.base_raster(C=3, H=150, W=203, dtype=np.uint8), 1)):
        for seg in (dict(tile=(64, 32)), dict(rows_per_strip=40)):
            for pred in (1, 2):
                lay = _layout(a, seg, planar, "deflate", pred)
                body, _, counts = H.host_encode(shim, a, lay)
                tiff_write.write_segments(path, lay, body, counts)
                try:
                    with Image.open(path) as im:
                        got = np.asarray(im)
                except Exception as e:      # noqa: BLE001
                    if "decoder" in str(e) and "not available" in str(e):
                        pytest.skip(f"this Pillow has no libtiff: {e}")
                    raise
                want = a[0] if a.shape[0] == 1 else a.transpose(1, 2, 0)
                assert got.shape == want.shape and np.array_equal(got.astype(a.dtype), want), (a.shape, seg, pred)


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_the_encoder_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "tiff_write_main")
    cmd = [H.cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "tiff_write_main.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "213 segments, 0 failed" in run.stdout and "ERROR" not in run.stderr
