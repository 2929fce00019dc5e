"""The TIFF reader on the CPU: lbdrn_hip/tiff.py's parser against the tables tests/tiff_reference.py's writer wrote, on every
layout; the reference decoders against files libtiff wrote (tests/golden/tiff_libtiff.npz); the host build of csrc/tiff.inc
-- through tests/tiff_host_shim.cpp, compiled by g++ into a temporary directory: the same text the device runs -- segment by
segment against the reference; the ValueErrors for everything outside the subset; the library's checks that come before any
launch; the kernels' resource usage; the host path of an oversize Deflate strip; raster_io.read_raster end to end with the device stage replaced by the
host shim; and tests/tiff_damage_main.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer, which feeds the host decoders damaged streams -- and, once each, the scene-sized segments of
tests/tiff_big_cases.py, sound and damaged (tests/test_tiff_host_big.py runs that table through the shim).  No GPU.  Every
comparison is exact."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tiff_reference as R  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
_shim = None

# every segmentation the GPU test uses, on a raster whose sides divide by none of them
SEGMENTATIONS = (dict(rows_per_strip=1), dict(rows_per_strip=8), dict(rows_per_strip=37), dict(tile=(16, 16)), dict(tile=(32, 16)))
COMPRESSIONS = (R.COMP_NONE, R.COMP_LZW, R.COMP_DEFLATE, R.COMP_DEFLATE_OLD, R.COMP_PACKBITS)


def base_raster(C=8, H=37, W=53, dtype=np.uint16, seed=5):
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.integers(-60, 61, (C, H, W)), axis=2) + rng.integers(0, 65536, (C, H, 1))
    a[:, 3, :] = rng.integers(0, 65536, (C, W))      # a row of noise
    a[:, 7:9, :] = 513                               # two constant rows
    return (a % (256 if np.dtype(dtype).itemsize == 1 else 65536)).astype(dtype)


def layouts():
    """a covering set: every segmentation x planar x compression x predictor, the byte order, container, band count and depth
    drawn per case from a seeded generator"""
    rng = np.random.default_rng(11)
    out = []
    for comp in COMPRESSIONS:
        for pred in (1, 2):
            for seg in SEGMENTATIONS:
                for planar in (1, 2):
                    out.append(dict(seg, planar=planar, compression=comp, predictor=pred, byteorder="<>"[int(rng.integers(2))],
                                    bigtiff=bool(rng.integers(2)), bands=(1, 3, 4, 8)[int(rng.integers(4))],
                                    dtype=(np.uint8, np.uint16)[int(rng.integers(2))]))
    return out


def layout_file(lay, **more):
    kw = {k: v for k, v in lay.items() if k not in ("bands", "dtype")}
    kw.update(more)
    a = base_raster(dtype=lay["dtype"])[:lay["bands"]]
    data, info = R.write_tiff(a, **kw)
    return a, data, info


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler (g++): the reader's host text cannot be compiled")
    return cxx


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        out = os.path.join(str(tmp_path_factory.mktemp("tiff_shim")), "libtiff_host_shim.so")
        subprocess.check_call([_cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                               os.path.join(ROOT, "tests", "tiff_host_shim.cpp")])
        L = ctypes.CDLL(out)
        L.tiff_shim_decode.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        L.tiff_shim_segment_count.argtypes = [ctypes.c_void_p]
        L.tiff_shim_segment_count.restype = ctypes.c_int64
        L.tiff_shim_expected.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        L.tiff_shim_expected.restype = ctypes.c_int64
        L.tiff_shim_cap.argtypes = [ctypes.c_int]
        L.tiff_shim_cap.restype = ctypes.c_uint64
        L.tiff_shim_adler32.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.tiff_shim_adler32.restype = ctypes.c_uint32
        _shim = L
    return _shim


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


def shim_decode(L, compression, data, expect):
    """(status, bytes): one segment through the host build of csrc/tiff.inc; 64 bytes behind the output must stay"""
    out = np.full(expect + 64, 0x77, np.uint8)
    st = L.tiff_shim_decode(8 if compression == R.COMP_DEFLATE_OLD else compression, bytes(data), len(data), out.ctypes.data, expect)
    assert (out[expect:] == 0x77).all(), "the decoder wrote behind the segment"
    return st, out[:expect].tobytes()


def shim_read(L, buf):
    """a whole file: lbdrn_hip.tiff's parser, the host build of the decoders, the reference's placement"""
    from lbdrn_hip import tiff
    sc = tiff.parse(buf)
    lay = sc.layout
    assert L.tiff_shim_segment_count(ctypes.byref(lay)) == len(sc.offsets)
    segs = []
    for i, (o, n) in enumerate(zip(sc.offsets.tolist(), sc.counts.tolist())):
        st, raw = shim_decode(L, lay.compression, buf[o:o + n], L.tiff_shim_expected(ctypes.byref(lay), i))
        assert st == 0, (i, st)
        segs.append(raw)
    return R.place_segments(segs, lay.C, lay.H, lay.W, np.uint8 if lay.bits == 8 else np.uint16,
                            tile=(lay.seg_w, lay.seg_h) if lay.tiled else None, rows_per_strip=lay.seg_h, planar=lay.planar,
                            predictor=lay.predictor, byteorder=">" if lay.big_endian else "<")


def golden_files(golden):
    g = golden["tiff_libtiff"]
    return [(k[:-len("__file")], g[k].tobytes(), g[k.split("_")[0] + "__pixels"]) for k in g.files if k.endswith("__file")]


# ---------------------------------------------------------------- the reference by itself, and against libtiff

def test_reference_codecs_round_trip_and_lzw_uses_every_width():
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 65536, 64 * 200).astype("<u2").tobytes()      # 25.6 KB
    for data in (noise, b"\x07" * 30000, b"a", bytes(range(256)) * 3 + b"\0" * 700 + b"abc" * 50):
        for mode in R.DEFLATE_MODES:
            assert R.decompress(R.deflate(data, mode), R.COMP_DEFLATE, len(data)) == data
        assert R.lzw_decode(R.lzw_encode(data), len(data)) == data
        assert R.packbits_decode(R.packbits_encode(data, 300), len(data)) == data
    # the noise strip clears the table several times: more codes than two tables hold
    stream = R.lzw_encode(noise)
    assert len(stream) * 8 / 12 > 2.5 * 4094 and len(stream) > len(noise)
    # Deflate's four forms are four different streams: stored, fixed and dynamic block types, and more than one block
    forms = {m: R.deflate(b"\x07" * 5000 + noise[:3000], m) for m in R.DEFLATE_MODES}
    assert [forms[m][2] & 7 for m in ("stored", "fixed", "dynamic")] == [1, 3, 5] and len(set(forms.values())) == 4


def test_reference_reads_what_libtiff_wrote(golden):
    files = golden_files(golden)
    assert len(files) == 20
    for name, buf, pixels in files:
        got = reference_read(buf)
        assert got.dtype == pixels.dtype and np.array_equal(got, pixels), name


def reference_read(buf):
    """a file through the product's parser and the reference's decoders and placement"""
    from lbdrn_hip import tiff
    sc = tiff.parse(buf)
    lay = sc.layout
    bps = lay.bits // 8
    spp = 1 if lay.planar == 2 else lay.C
    grid = R.segment_grid(lay.C, lay.H, lay.W, (lay.seg_w, lay.seg_h) if lay.tiled else None, lay.seg_h, lay.planar)
    segs = []
    for (o, n), (_, _, _, sh, sw, rows) in zip(zip(sc.offsets.tolist(), sc.counts.tolist()), grid):
        segs.append(R.decompress(buf[o:o + n], lay.compression, (sh if lay.tiled else rows) * sw * spp * bps))
    return R.place_segments(segs, lay.C, lay.H, lay.W, np.uint8 if lay.bits == 8 else np.uint16,
                            tile=(lay.seg_w, lay.seg_h) if lay.tiled else None, rows_per_strip=lay.seg_h, planar=lay.planar,
                            predictor=lay.predictor, byteorder=">" if lay.big_endian else "<")


# ---------------------------------------------------------------- the parser

def test_parser_finds_the_writers_tables_on_every_layout():
    from lbdrn_hip import tiff
    seen = set()
    for lay in layouts():
        if lay["compression"] == R.COMP_LZW and lay["bands"] * np.dtype(lay["dtype"]).itemsize > 8:
            lay = dict(lay, bands=3)      # (the Python LZW encoder is what takes the time here)
        a, data, info = layout_file(lay)
        sc = tiff.parse(data)
        L = sc.layout
        assert sc.offsets.tolist() == info["offsets"] and sc.counts.tolist() == info["counts"], lay
        assert (L.C, L.H, L.W, L.bits) == (a.shape[0], 37, 53, a.dtype.itemsize * 8)
        assert L.big_endian == (lay["byteorder"] == ">") and L.planar == lay["planar"]
        assert L.compression == (8 if lay["compression"] == R.COMP_DEFLATE_OLD else lay["compression"])
        assert L.predictor == info["predictor"]      # as libtiff: honoured with LZW and Deflate only
        assert L.tiled == ("tile" in lay)
        assert (L.seg_w, L.seg_h) == (lay["tile"] if "tile" in lay else (53, lay["rows_per_strip"]))
        assert struct.unpack_from(lay["byteorder"] + "H", data, 2)[0] == (43 if lay["bigtiff"] else 42)
        assert np.array_equal(reference_read(data), a), lay
        seen.add((lay["byteorder"], lay["bigtiff"], lay["bands"], lay["dtype"]))
    assert {s[0] for s in seen} == {"<", ">"} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {1, 3, 4, 8}


def test_value_errors_name_the_tag_and_value():
    from lbdrn_hip import tiff
    a = base_raster()[:2]

    def refused(match, **kw):
        data, _ = R.write_tiff(a, **kw)
        with pytest.raises(ValueError, match=match):
            tiff.parse(data, "scene.tif")
    for comp in (7, 50000, 34887, 6, 2):      # JPEG, ZSTD, LERC, old JPEG, CCITT
        data, _ = R.write_tiff(a, compression=R.COMP_NONE)
        at = data.index(struct.pack("<HHIH", 259, 3, 1, 1))
        bad = data[:at + 8] + struct.pack("<H", comp) + data[at + 10:]
        with pytest.raises(ValueError, match=rf"Compression \(259\) = {comp}"):
            tiff.parse(bad, "scene.tif")
    refused(r"Predictor \(317\) = 3", compression=R.COMP_LZW, predictor=3)
    refused(r"SampleFormat \(339\) = 2", compression=R.COMP_DEFLATE, sample_format=2)
    refused(r"SampleFormat \(339\) = 3", tile=(16, 16), sample_format=3)
    for bits in (1, 4, 12, 32):
        data, _ = R.write_tiff(a, tile=(16, 16))
        at = data.index(struct.pack("<HHIHH", 258, 3, 2, 16, 16))
        with pytest.raises(ValueError, match=rf"BitsPerSample \(258\) = {bits}"):
            tiff.parse(data[:at + 8] + struct.pack("<HH", bits, bits) + data[at + 12:], "scene.tif")
    data, _ = R.write_tiff(a, tile=(16, 16))
    at = data.index(struct.pack("<HHIHH", 258, 3, 2, 16, 16))
    with pytest.raises(ValueError, match=r"BitsPerSample \(258\) = \[16, 8\]"):
        tiff.parse(data[:at + 8] + struct.pack("<HH", 16, 8) + data[at + 12:], "scene.tif")
    # old-style LZW, as libtiff detects it: first byte 0, bit 0 of the second set
    with pytest.raises(ValueError, match=r"Compression \(259\) = 5.*old-style"):
        tiff.parse(R.write_tiff(a, compression=R.COMP_LZW, segment_hook=lambda i, p: b"\x00\x01" + p[2:] if i == 1 else p)[0], "scene.tif")
    # a table that leaves the file, a table of the wrong length, no TIFF at all
    data, info = R.write_tiff(a, compression=R.COMP_DEFLATE, rows_per_strip=8)
    with pytest.raises(ValueError, match=r"StripOffsets \(273\)"):
        tiff.parse(_cut_last_segment(data, info), "scene.tif")
    for junk in (b"", b"II", b"PK\x03\x04" + bytes(64), b"II\x2c\x00" + bytes(64)):
        with pytest.raises(ValueError, match="not a TIFF"):
            tiff.parse(junk, "scene.tif")


def _cut_last_segment(data, info):
    """the same file with the last segment's byte count grown past the file's end"""
    want = struct.pack("<I", info["counts"][-1])
    at = data.rindex(struct.pack("<%dI" % len(info["counts"]), *info["counts"]))
    at += 4 * (len(info["counts"]) - 1)
    assert data[at:at + 4] == want
    return data[:at] + struct.pack("<I", len(data)) + data[at + 4:]


# ---------------------------------------------------------------- the host build of csrc/tiff.inc

def test_host_build_equals_the_reference_segment_by_segment(shim, golden):
    from lbdrn_hip import tiff
    n = 0
    for name, buf, pixels in golden_files(golden):
        sc = tiff.parse(buf)
        lay = sc.layout
        for i, (o, c) in enumerate(zip(sc.offsets.tolist(), sc.counts.tolist())):
            expect = shim.tiff_shim_expected(ctypes.byref(lay), i)
            st, raw = shim_decode(shim, lay.compression, buf[o:o + c], expect)
            assert st == 0 and raw == R.decompress(buf[o:o + c], lay.compression, expect), (name, i)
            n += 1
        assert np.array_equal(shim_read(shim, buf), pixels), name
    assert n == 28      # sixteen and seven one-strip files, five strips of 64 rows
    for lay in layouts():
        if lay["compression"] == R.COMP_LZW and lay["bands"] * np.dtype(lay["dtype"]).itemsize > 8:
            lay = dict(lay, bands=3)
        for mode in (R.DEFLATE_MODES if lay["compression"] == R.COMP_DEFLATE and lay["predictor"] == 2 else ("dynamic",)):
            a, data, info = layout_file(lay, deflate_mode=mode)
            sc = tiff.parse(data)
            for i, (o, c) in enumerate(zip(info["offsets"], info["counts"])):
                assert shim.tiff_shim_expected(ctypes.byref(sc.layout), i) == len(info["raw"][i])
                assert shim_decode(shim, lay["compression"], data[o:o + c], len(info["raw"][i])) == (0, info["raw"][i]), (lay, i)
            assert np.array_equal(shim_read(shim, data), a), lay


def test_host_build_on_the_codecs_hard_cases(shim):
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 65536, 64 * 200).astype("<u2").tobytes()
    const = b"\x21" * 40000
    for data in (noise, const, b"a", b"ab" * 5000, bytes(300000)):
        assert shim_decode(shim, R.COMP_LZW, R.lzw_encode(data), len(data)) == (0, data)
        for mode in R.DEFLATE_MODES:
            assert shim_decode(shim, R.COMP_DEFLATE, R.deflate(data, mode), len(data)) == (0, data)
        assert shim_decode(shim, R.COMP_PACKBITS, R.packbits_encode(data, 1000), len(data)) == (0, data)
        assert shim.tiff_shim_adler32(data, len(data)) == __import__("zlib").adler32(data)
    # decoding stops at the expected size: a stream that holds more is read as far as the segment goes
    for comp in (R.COMP_LZW, R.COMP_DEFLATE):
        assert shim_decode(shim, comp, R.compress(noise, comp), 1000) == (0, noise[:1000])
    # PackBits: literal and replicate runs of exactly 128, and the no-op byte
    data = bytes(range(128)) + b"\x05" * 128 + bytes(range(100, 228)) + b"\x09" * 128
    stream = R.packbits_encode(data)
    assert stream[0] == 127 and stream[129] == 0x81 and len(stream) == 2 * 129 + 2 * 2
    assert shim_decode(shim, R.COMP_PACKBITS, stream, len(data)) == (0, data)
    assert shim_decode(shim, R.COMP_PACKBITS, b"\x80" + stream[:129] + b"\x80\x80" + stream[129:] + b"\x80", len(data)) == (0, data)


def test_the_fixed_damage_list_ends_in_a_status_every_time(shim):
    a = base_raster()[:1]
    raw = R.raw_segments(a, rows_per_strip=8, predictor=2)[1]
    for comp in (R.COMP_DEFLATE, R.COMP_LZW, R.COMP_PACKBITS):
        cases = R.damage_cases(comp, R.compress(raw, comp, row_bytes=106), len(raw))
        assert 19 <= len(cases) <= 22
        for name, bad in cases:
            st, _ = shim_decode(shim, comp, bad, len(raw))
            assert st != 0, (comp, name)
            with pytest.raises(Exception):
                R.decompress(bad, comp, len(raw))


# ---------------------------------------------------------------- the library's checks that come before any launch

def test_library_refuses_before_any_launch():
    from lbdrn_hip import tiff
    L = tiff.lib()
    lay = tiff.Layout(8, 37, 53, 16, 0, 2, 53, 1, 0, tiff.COMP_LZW, 2)
    assert L.lbdrn_tiff_abi_version() == 1
    assert L.lbdrn_tiff_segment_count(ctypes.byref(lay)) == 296
    assert L.lbdrn_tiff_workspace(ctypes.byref(lay)) >= 296 * (16 + 106)
    assert [L.lbdrn_tiff_segment_cap(c) > 0 for c in (1, 5, 8, 32773, 7, 32946)] == [True] * 4 + [False] * 2
    for field, value in (("C", 0), ("bits", 12), ("planar", 3), ("seg_w", 52), ("seg_h", 38), ("compression", 7), ("predictor", 3),
                         ("W", (1 << 20) + 1), ("big_endian", 2)):
        bad = tiff.Layout(*[getattr(lay, n) for n, _ in tiff.Layout._fields_])
        setattr(bad, field, value)
        assert L.lbdrn_tiff_segment_count(ctypes.byref(bad)) == 0 and L.lbdrn_tiff_workspace(ctypes.byref(bad)) == 0, field
    offsets = np.arange(296, dtype=np.uint64) * 10 + 8
    counts = np.full(296, 10, np.uint64)
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before any device work

    def call(lay, nbytes, offsets, counts, nseg, ws_bytes):
        return L.lbdrn_tiff_decode(ctypes.byref(lay), fake, nbytes, offsets.ctypes.data, counts.ctypes.data, nseg, fake, fake, fake, ws_bytes, None)
    assert call(lay, 4000, offsets, counts, 295, 1 << 30) == tiff.E_ARG and b"segments" in L.lbdrn_tiff_last_error()
    assert call(lay, 2967, offsets, counts, 296, 1 << 30) == tiff.E_ARG and b"segment 295" in L.lbdrn_tiff_last_error()
    wrap = offsets.copy()
    wrap[7] = np.uint64(2 ** 64 - 5)
    assert call(lay, 4000, wrap, counts, 296, 1 << 30) == tiff.E_ARG and b"segment 7" in L.lbdrn_tiff_last_error()
    assert call(lay, 4000, offsets, counts, 296, L.lbdrn_tiff_workspace(ctypes.byref(lay)) - 1) == tiff.E_WORKSPACE
    big = tiff.Layout(1, 1 << 15, 1 << 15, 16, 0, 2, 1 << 15, 1 << 15, 0, tiff.COMP_LZW, 1)      # one strip of 2 GB
    one = np.array([8], np.uint64)
    assert call(big, 4000, one, one, 1, 1 << 40) == tiff.E_UNSUPPORTED and b"cap" in L.lbdrn_tiff_last_error()


def test_no_kernel_of_the_library_has_scratch_or_spilled_registers():
    """the code objects' metadata, read as scripts/kernel_resources.py reads it: Huffman tables, the history ring and the LZW
    table are in LDS, nothing is in private memory.  (k_tiff_inflate keeps more wave-uniform values than there are scalar
    registers; the compiler parks some in lanes of a vector register -- sgpr_spill_count -- which is no memory traffic.)"""
    from lbdrn_hip import tiff
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    if not os.path.exists(os.path.join(KR.LLVM, "llvm-objdump")) or not os.path.exists(tiff._PATH):
        pytest.skip("llvm-objdump or the library is missing")
    rows = KR.kernel_resources(tiff._PATH)
    names = " ".join(r["demangled"] for r in rows)
    assert all(k in names for k in ("k_tiff_inflate", "k_tiff_lzw", "k_tiff_packbits", "k_tiff_place")) and len(rows) == 5
    for r in rows:
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0 and r["lds"] <= 65536, r      # (as tests/test_kernel_disassembly.py asks of liblbdrn_hip.so)


# ---------------------------------------------------------------- host paths

def test_oversize_deflate_strip_takes_the_host_path_and_other_codecs_name_the_cap(tmp_path):
    from lbdrn_hip import raster_io, tiff
    cap = tiff.lib().lbdrn_tiff_segment_cap(tiff.COMP_DEFLATE)
    W = 2048
    H = cap // (2 * W) + 1      # one strip per band, one row above the cap
    a = ((np.arange(W, dtype=np.uint32)[None, None, :] * 3 + np.arange(H, dtype=np.uint32)[None, :, None] * 5 +
          np.arange(2, dtype=np.uint32)[:, None, None] * 1000) % 65536).astype(np.uint16)
    data, _ = R.write_tiff(a, compression=R.COMP_DEFLATE, predictor=2, planar=2, deflate_mode="fixed", byteorder=">")
    path = str(tmp_path / "one_strip.tif")
    with open(path, "wb") as f:
        f.write(data)
    got = raster_io.read_raster(path)      # no device: zlib on the host
    assert got.dtype == np.uint16 and np.array_equal(got, a)
    for comp in (R.COMP_LZW, R.COMP_PACKBITS):      # (the parser takes the layout; the stand-in stream is never decoded)
        cap = tiff.lib().lbdrn_tiff_segment_cap(comp)
        H = cap // (2 * W) + 1
        fake, _ = R.write_tiff(np.zeros((1, H, W), np.uint16), compression=R.COMP_NONE)
        at = fake.index(struct.pack("<HHIH", 259, 3, 1, 1))
        fake = fake[:at + 8] + struct.pack("<H", comp) + fake[at + 10:]
        with open(path, "wb") as f:
            f.write(fake)
        with pytest.raises(ValueError, match=rf"above the cap of {cap} bytes"):
            raster_io.read_raster(path)


def test_read_raster_end_to_end_with_the_device_stage_on_the_host(shim, tmp_path, monkeypatch):
    """raster_io.read_raster on a tiled Deflate file, with tiff.read replaced by the host build of the same decoders: what the
    uncompressed twin gives, band for band -- and a one-band file comes back [H,W], as _read_tiff returns it"""
    from lbdrn_hip import raster_io, tiff
    if raster_io._gdal() is not None:
        pytest.skip("GDAL reads the file first here")

    def host_read(path, device=None):
        with open(path, "rb") as f:
            a = shim_read(shim, f.read())
        return a[0] if a.shape[0] == 1 else a
    monkeypatch.setattr(tiff, "read", host_read)
    for bands in (4, 1):
        a = base_raster(C=bands, H=47, W=51)
        plain, packed = str(tmp_path / f"plain{bands}.tif"), str(tmp_path / f"packed{bands}.tif")
        raster_io.write_raster(plain, a)
        with open(packed, "wb") as f:
            f.write(R.write_tiff(a, bigtiff=True, tile=(16, 16), planar=1, predictor=2, compression=R.COMP_DEFLATE)[0])
        one, two = raster_io.read_raster(plain), raster_io.read_raster(packed)
        assert one.shape == two.shape == ((bands, 47, 51) if bands > 1 else (47, 51)) and one.dtype == two.dtype == np.uint16
        assert np.array_equal(one, two) and np.array_equal(two.reshape(a.shape), a)


def test_without_a_device_a_compressed_file_raises_the_no_cpu_path_error(tmp_path):
    import torch
    from lbdrn_hip import raster_io, tiff
    if torch.cuda.is_available() or raster_io._gdal() is not None:
        pytest.skip("a device (or GDAL) is present")
    path = str(tmp_path / "t.tif")
    with open(path, "wb") as f:
        f.write(R.write_tiff(base_raster()[:2], tile=(16, 16), compression=R.COMP_LZW)[0])
    with pytest.raises(tiff.TiffError, match="no CPU path"):
        raster_io.read_raster(path)
    with pytest.raises(tiff.TiffError, match="no CPU path"):
        raster_io.read_raster_device(path, "cuda:0")


# ---------------------------------------------------------------- the sanitizer run: a program of its own

def test_damaged_segments_under_sanitizers_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "tiff_damage")
    cmd = [_cxx(), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), "-o", exe, os.path.join(ROOT, "tests", "tiff_damage_main.cpp")]
    # does this compiler have the sanitizers' runtimes at all?  Asked of an empty program with the same flags, before the
    # program under test is touched: a failure of the real build below is then a failure, whatever its text.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = [f for f in cmd[1:cmd.index("-o")] if not f.startswith("-I")]
    if subprocess.run([cmd[0]] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this host compiler cannot build an empty program with -fsanitize=address,undefined (no runtimes)")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # the cases: sound streams of every codec and Deflate form, and the fixed damage list the GPU test runs on the device
    rng = np.random.default_rng(6)
    smooth = (np.cumsum(rng.integers(-3, 4, 6000)) % 65536).astype("<u2").tobytes()
    noise = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    recs = []

    def rec(kind, comp, expect, stream, want=b""):
        recs.append(struct.pack("<IIII", kind, comp, expect, len(stream)) + stream + want)
    for mode in R.DEFLATE_MODES:
        rec(1, R.COMP_DEFLATE, len(smooth), R.deflate(smooth, mode), smooth)
    rec(1, R.COMP_DEFLATE, len(noise), R.deflate(noise), noise)
    for data in (smooth, noise, b"\x21" * 5000):
        rec(1, R.COMP_LZW, len(data), R.lzw_encode(data), data)
        rec(1, R.COMP_PACKBITS, len(data), R.packbits_encode(data, 500), data)
    raw = R.raw_segments(base_raster()[:1], rows_per_strip=8, predictor=2)[1]
    nfixed = 0
    for comp in (R.COMP_DEFLATE, R.COMP_LZW, R.COMP_PACKBITS):
        for _, bad in R.damage_cases(comp, R.compress(raw, comp, row_bytes=106), len(raw)):
            rec(2, comp, len(raw), bad)
            nfixed += 1
    # segments of a scene's size (tests/tiff_big_cases.py): every sound row once, and the damaged large segments
    import tiff_big_cases as B
    for _, comp, stream, want in B.rows():
        rec(3, comp, len(want), stream, want)
    for _, comp, bad, _, _, want in B.damage_rows():
        rec(2, comp, len(want), bad)
        nfixed += 1
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(recs))
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    nsound = sum(r[0] in (1, 3) for r in recs)
    assert nsound == 11 + len(B.rows())
    assert f"{nsound} sound streams, {nfixed} of the fixed list flagged" in run.stdout and "ERROR" not in run.stderr
