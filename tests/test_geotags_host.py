"""A scene's georeferencing and nodata tags through the .bin, on the host: the 'LBGT' chunk (lbdrn_hip.geotags.pack / unpack),
its place in the container beside the residual-layer trailer, the move of the tags under a crop (geotags.shift) against the
formulas written out here, raster_io.read_geo_tags through a buffer that records what is asked of it, encode.py / sweep.py
--keep-tags with the device work replaced by stand-ins (as tests/test_cli_sharding_cpu.py and tests/test_resid_sharding_cpu.py
do it), and python -m lbdrn_hip.geotags --attach / --strip.  No GPU."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
for p in (PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tiff_reference as TR  # noqa: E402
from pyramid_helpers import GEO, with_tags  # noqa: E402
from test_cli_sharding_cpu import _records, _stub_report, _stub_train_tiles  # noqa: E402
from test_resid_sharding_cpu import _stub_layer  # noqa: E402
from test_sweep_in_flight_host import _stub_train_tiles_at  # noqa: E402
from test_sweep_in_flight_host import _stub_train_tiles as _stub_train_tiles_k  # noqa: E402

ELEMENT = {33550: (12, 8), 33922: (12, 8), 34264: (12, 8), 34735: (3, 2), 34736: (12, 8), 34737: (2, 1), 42112: (2, 1), 42113: (2, 1)}


def d(*vals):
    return struct.pack("<%dd" % len(vals), *vals)


def doubles(raw):
    return struct.unpack("<%dd" % (len(raw) // 8), raw)


def random_tags(rng):
    """a tag list over a random subset of the eight tags (all of them every fourth time), random counts and values"""
    tags = []
    for tag, (typ, size) in ELEMENT.items():
        if rng.integers(0, 4) and rng.integers(0, 2):
            continue
        cnt = int(rng.integers(1, 40))
        if typ == 2:
            raw = bytes(rng.integers(32, 127, cnt - 1, dtype=np.uint8)) + b"\0"
        elif typ == 3:
            raw = rng.integers(0, 65536, cnt, dtype=np.uint16).astype("<u2").tobytes()
        else:
            raw = (rng.standard_normal(cnt) * 10.0 ** rng.integers(-3, 8)).astype("<f8").tobytes()
        tags.append((tag, typ, cnt, raw))
    return tags


# ---------------------------------------------------------------- the chunk

def test_chunk_round_trip_and_the_compression_flag():
    from lbdrn_hip import geotags, tiff
    assert ELEMENT == tiff.GEO_TAGS
    rng = np.random.default_rng(11)
    lists = [random_tags(rng) for _ in range(40)] + [list(GEO), []]
    assert any(len(t) == 8 for t in lists)
    for tags in lists:
        chunk = geotags.pack(tags)
        assert chunk == geotags.pack(tags) == geotags.pack(list(reversed(tags)))      # a function of the tag list alone
        assert geotags.unpack(chunk) == tags
        magic, version, flags, reserved, n = struct.unpack_from(">4sBBHI", chunk, 0)
        assert (magic, version, reserved, flags & ~1, 12 + n + 4) == (b"LBGT", 1, 0, 0, len(chunk))
        raw = struct.pack(">H", len(tags)) + b"".join(struct.pack(">HHI", t, ty, c) + v for t, ty, c, v in tags)
        assert struct.unpack_from(">I", chunk, 12 + n)[0] == zlib.crc32(raw)
        assert chunk[12:12 + n] == (zlib.compress(raw, 9) if flags else raw)
        assert bool(flags) == (len(zlib.compress(raw, 9)) < len(raw))
    # 5 KB of GDAL_METADATA: compressed; a pixel scale of three doubles: not
    xml = ("<GDALMetadata>\n" + "".join(f'  <Item name="LINE_NUM_COEFF_{k}" domain="RPC">{k * 1.25e-7!r}</Item>\n' for k in range(80))
           ).encode("ascii")
    xml = (xml * (5000 // len(xml) + 1))[:4985] + b"</GDALMetadata>"
    assert len(xml) == 5000
    big = [(42112, 2, len(xml) + 1, xml + b"\0")]
    chunk = geotags.pack(big)
    assert chunk[5] == 1 and len(chunk) < 2500 and geotags.unpack(chunk) == big
    small = [(33550, 12, 3, d(29.98134, 30.01267, 0.0))]
    chunk = geotags.pack(small)
    assert chunk[5] == 0 and len(chunk) == 16 + 2 + 8 + 24 and geotags.unpack(chunk) == small


def test_pack_refuses_what_no_chunk_carries():
    from lbdrn_hip import geotags
    good = (33550, 12, 3, d(1.0, 1.0, 0.0))
    for bad in ([(256, 4, 1, b"\0\0\0\0")],                      # a tag outside GEO_TAGS
                [(33550, 5, 3, d(1.0, 1.0, 0.0))],               # another type than the tag's
                [good, good],                                    # twice
                [(33550, 12, 3, d(1.0, 1.0))],                   # 16 bytes for three doubles
                [(34735, 3, 4, b"\0" * 7)],
                [(42113, 2, 0, b"")],                            # nothing a TIFF entry holds
                [(33550, 12, 3)]):
        with pytest.raises(ValueError):
            geotags.pack(bad)


def test_every_truncation_and_every_substituted_byte_is_refused():
    """One chunk of 120 bytes, stored uncompressed: each of its proper prefixes and each of its 120 x 255 single-byte
    substitutions raises ValueError.  A compressed one: every truncation raises; a substitution raises or -- the padding bits
    behind a Deflate stream's last code, the level bits of the zlib header -- reads the very same list, never another."""
    from lbdrn_hip import geotags
    tags = [(33550, 12, 3, d(29.98134, 30.01267, 1.0037)), (33922, 12, 6, d(0.53, 0.21, 0.127, 399960.37, 5700000.52, 123.456)),
            (42113, 2, 6, b"65535\0")]
    chunk = geotags.pack(tags)
    assert len(chunk) == 120 and chunk[5] == 0 and geotags.unpack(chunk) == tags
    ran = 0
    for n in range(len(chunk)):
        with pytest.raises(ValueError):
            geotags.unpack(chunk[:n])
        ran += 1
    for at in range(len(chunk)):
        for v in range(256):
            if v != chunk[at]:
                with pytest.raises(ValueError):
                    geotags.unpack(chunk[:at] + bytes([v]) + chunk[at + 1:])
                ran += 1
    assert ran == len(chunk) + 255 * len(chunk)
    with pytest.raises(ValueError):
        geotags.unpack(chunk + b"\0")
    with pytest.raises(ValueError):
        geotags.unpack(chunk + chunk)
    packed = geotags.pack([(34737, 2, 120, b"WGS 84 / UTM zone 32N|" * 5 + b"123456789\0")])
    assert len(packed) <= 200 and packed[5] == 1
    want, ran = geotags.unpack(packed), 0
    for n in range(len(packed)):
        with pytest.raises(ValueError):
            geotags.unpack(packed[:n])
    for at in range(len(packed)):
        for v in range(256):
            if v != packed[at]:
                try:
                    got = geotags.unpack(packed[:at] + bytes([v]) + packed[at + 1:])
                except ValueError:
                    got = None
                assert got is None or (got == want and 12 <= at < len(packed) - 4), (at, v)      # never in the framing or the CRC
                ran += 1
    assert ran == 255 * len(packed)


def test_unpack_refuses_reordered_unknown_and_ill_sized_tags():
    """payloads with a right CRC that pack() would never have written"""
    from lbdrn_hip import geotags

    def chunk_of(raw, flags=0, version=1, reserved=0):
        return b"LBGT" + struct.pack(">BBHI", version, flags, reserved, len(raw)) + raw + struct.pack(">I", zlib.crc32(raw))
    e = lambda tag, typ, cnt, val: struct.pack(">HHI", tag, typ, cnt) + val
    a, b = e(33550, 12, 3, d(1.0, 1.0, 0.0)), e(42113, 2, 2, b"0\0")
    assert geotags.unpack(chunk_of(struct.pack(">H", 2) + a + b)) == [(33550, 12, 3, d(1.0, 1.0, 0.0)), (42113, 2, 2, b"0\0")]
    for raw in (struct.pack(">H", 2) + b + a,                                  # out of order
                struct.pack(">H", 2) + a + a,                                  # twice
                struct.pack(">H", 1) + e(256, 4, 1, b"\0\0\0\0"),              # no geo tag
                struct.pack(">H", 1) + e(33550, 5, 3, d(1.0, 1.0, 0.0)),       # another type
                struct.pack(">H", 1) + e(33550, 12, 4, d(1.0, 1.0, 0.0)),      # the values end behind the payload
                struct.pack(">H", 1) + a + b"\0",                              # bytes behind the last tag
                struct.pack(">H", 3) + a + b,                                  # fewer tags than counted
                struct.pack(">H", 1) + e(42113, 2, 0, b""),
                b"\0"):
        with pytest.raises(ValueError):
            geotags.unpack(chunk_of(raw))
    ok = struct.pack(">H", 1) + a
    for kw in (dict(version=2), dict(version=0), dict(reserved=1), dict(flags=2), dict(flags=0x80), dict(flags=1)):
        with pytest.raises(ValueError):
            geotags.unpack(chunk_of(ok, **kw))
    # flag bit 0 over a stream that is no shorter than what it holds: pack() sets it exactly when the stream is shorter
    dense = struct.pack(">H", 1) + e(33550, 12, 3, d(29.98134, 30.01267, 1.0037))
    z = zlib.compress(dense, 9)
    assert len(z) >= len(dense) and geotags.unpack(chunk_of(dense)) == [(33550, 12, 3, d(29.98134, 30.01267, 1.0037))]
    with pytest.raises(ValueError):
        geotags.unpack(b"LBGT" + struct.pack(">BBHI", 1, 1, 0, len(z)) + z + struct.pack(">I", zlib.crc32(dense)))


# ---------------------------------------------------------------- the container

def _files(act="sine"):
    from lbdrn_hip import container
    nn, base = [b"n" * 11, b"N" * 7, b"n" * 5, b"n" * 3], [b"b" * 13, b"B" * 2, b"b" * 9, b"b" * 1]
    header = container.pack_header(2, 300, 200, 5, 64, 2, 2, [len(x) for x in nn], [len(x) for x in base], activation=act)
    plain = header + b"".join(a + b for a, b in zip(nn, base))
    bodies = [b"LBR1" + bytes([k]) * (5 * k) for k in range(4)]
    return plain, container.pack_residual_trailer(3, bodies), bodies


def test_container_places_the_chunk_behind_everything():
    from lbdrn_hip import container, geotags
    for act in ("sine", "relu"):
        plain, trailer, bodies = _files(act)
        chunk = container.pack_geo_trailer(GEO)
        assert chunk == geotags.pack(GEO) and chunk[:4] == b"LBGT"
        full = plain + trailer
        for buf, layer, tags in ((plain, None, None), (plain + chunk, None, GEO), (full, (3, bodies), None), (full + chunk, (3, bodies), GEO)):
            assert container.unpack_residual_trailer(buf) == layer
            assert container.unpack_geo_trailer(buf) == tags
            assert container.unpack_header(buf) == container.unpack_header(plain)
            assert container.residual_trailer_offset(buf) == len(plain)
            assert container.strip_geo_trailer(buf) == (buf if tags is None else buf[:-len(chunk)])
        # what tests/test_resid_host.py lists stays refused, by both functions, with and without a chunk behind it
        refused = [full[:-1], full + b"\0", plain + b"LBRX" + trailer[4:], plain + b"LBRT\x02" + trailer[5:], plain[:-1]]
        refused += [bad + chunk for bad in refused[:4]]
        # the chunk in front of the trailer, two chunks, a byte behind the chunk, a damaged chunk
        refused += [plain + chunk + trailer, plain + chunk + chunk, full + chunk + chunk, plain + chunk + b"\0", full + chunk + b"\0",
                    full + chunk[:-1], plain + chunk[:-1], full + chunk[:20] + b"\xff" + chunk[21:], full + b"LBGU" + chunk[4:]]
        for bad in refused:
            for fn in (container.unpack_residual_trailer, container.unpack_geo_trailer, container.strip_geo_trailer):
                with pytest.raises(ValueError):
                    fn(bad)


# ---------------------------------------------------------------- shift

def _tag(tags, number):
    return [t for t in tags if t[0] == number][0]


def test_shift_tiepoint_with_a_pixel_scale():
    from lbdrn_hip import geotags
    rng = np.random.default_rng(5)
    for k in range(200):
        Sx, Sy = float(rng.uniform(0.1, 30.0)), float(rng.uniform(0.1, 30.0))
        I, J, K, X, Y, Z = (float(v) for v in rng.standard_normal(6) * 1e6)
        x0, y0 = int(rng.integers(0, 20000)), int(rng.integers(0, 20000))
        tags = [(33550, 12, 3, d(Sx, Sy, 0.0)), (33922, 12, 6, d(I, J, K, X, Y, Z))] + [t for t in GEO if t[0] > 34264]
        got = geotags.shift(tags, x0, y0)
        assert _tag(got, 33922) == (33922, 12, 6, d(I, J, K, X + x0 * Sx, Y - y0 * Sy, Z))      # equal to the bit
        assert [t for t in got if t[0] != 33922] == [t for t in tags if t[0] != 33922]             # the rest verbatim
    # the number gdal_translate -srcwin 100 200 ... carries for a 10 m grid
    got = geotags.shift(GEO[:2], 100, 200)
    assert doubles(got[1][3]) == (0.0, 0.0, 0.0, 399960.0 + 1000.0, 5700000.5 - 2000.0, 0.0) and got[0] == GEO[0]


def test_shift_other_tiepoints_move_their_raster_coordinates():
    from lbdrn_hip import geotags
    rng = np.random.default_rng(6)
    for n, with_scale in ((1, False), (2, True), (4, False), (9, True)):
        v = [float(x) for x in rng.standard_normal(6 * n) * 1e5]
        x0, y0 = int(rng.integers(1, 9000)), int(rng.integers(1, 9000))
        tags = ([(33550, 12, 3, d(2.0, 2.0, 0.0))] if with_scale else []) + [(33922, 12, 6 * n, d(*v)), GEO[3], GEO[7]]
        want = list(v)
        for k in range(n):
            want[6 * k], want[6 * k + 1] = v[6 * k] - x0, v[6 * k + 1] - y0
        got = geotags.shift(tags, x0, y0)
        assert _tag(got, 33922) == (33922, 12, 6 * n, d(*want))
        assert [t for t in got if t[0] != 33922] == [t for t in tags if t[0] != 33922]


def test_shift_transformation_and_both_tags_each_by_its_own_rule():
    from lbdrn_hip import geotags
    rng = np.random.default_rng(7)
    for k in range(100):
        M = [float(x) for x in rng.standard_normal(16) * 10.0 ** rng.integers(-2, 6)]
        x0, y0 = int(rng.integers(0, 30000)), int(rng.integers(0, 30000))
        want = list(M)
        for r in range(3):
            want[4 * r + 3] = (M[4 * r + 3] + M[4 * r] * x0) + M[4 * r + 1] * y0
        tie = d(0.0, 0.0, 0.0, 500000.0, 4100000.0, 0.0)
        tags = [(33550, 12, 3, d(0.5, 0.25, 0.0)), (33922, 12, 6, tie), (34264, 12, 16, d(*M)), GEO[3], GEO[6]]
        got = geotags.shift(tags, x0, y0)
        assert _tag(got, 34264) == (34264, 12, 16, d(*want)) and want[12:] == M[12:]
        assert _tag(got, 33922) == (33922, 12, 6, d(0.0, 0.0, 0.0, 500000.0 + x0 * 0.5, 4100000.0 - y0 * 0.25, 0.0))
        assert [got[0], got[3], got[4]] == [tags[0], tags[3], tags[4]]
        alone = geotags.shift([tags[2]], x0, y0)
        assert alone == [_tag(got, 34264)]


def test_shift_identity_and_composition():
    from lbdrn_hip import geotags
    rng = np.random.default_rng(8)
    # (0, 0): the bytes, whatever they are -- a negative zero, an infinity, a NaN payload
    odd = [(33550, 12, 3, d(float("inf"), float("nan"), -0.0)), (33922, 12, 6, d(-0.0, 0.0, 0.0, -0.0, float("nan"), 1.0)),
           (34264, 12, 16, d(*([-0.0] * 12 + [0.0, 0.0, 0.0, 1.0])))]
    for tags in (list(GEO), odd, [], [random_tags(rng) for _ in range(5)][-1]):
        assert geotags.shift(tags, 0, 0) == tags
    # exactly representable scales and origins: two moves are the move by the sum, in all three forms
    M = [2.0, 0.5, 0.0, 1024.0, -0.25, -4.0, 0.0, 65536.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    forms = ([(33550, 12, 3, d(0.5, 0.25, 0.0)), (33922, 12, 6, d(0.0, 0.0, 0.0, 4096.0, 8192.0, 0.0))],
             [(33922, 12, 12, d(0.0, 0.0, 0.0, 10.0, 20.0, 0.0, 100.0, 50.0, 0.0, 30.0, 40.0, 0.0))],
             [(34264, 12, 16, d(*M))],
             [(33550, 12, 3, d(4.0, 4.0, 0.0)), (33922, 12, 6, d(0.0, 0.0, 0.0, 3.0, 5.0, 0.0)), (34264, 12, 16, d(*M)), GEO[7]])
    for tags in forms:
        for _ in range(50):
            a, b, c, e = (int(v) for v in rng.integers(0, 4000, 4))
            assert geotags.shift(geotags.shift(tags, a, b), c, e) == geotags.shift(tags, a + c, b + e)


def test_stored_nodata_is_an_integer_sample_value_or_nothing():
    from lbdrn_hip import geotags
    nd = lambda text: [(42113, 2, len(text) + 1, text.encode() + b"\0")]
    assert geotags.stored_nodata(nd("0"), 16) == 0 and geotags.stored_nodata(nd("65535"), 16) == 65535
    assert geotags.stored_nodata(nd("255"), 8) == 255 and geotags.stored_nodata(nd("256"), 8) is None
    for text in ("65536", "-1", "nan", "0.5", "-9999", "1e3", ""):
        assert geotags.stored_nodata(nd(text), 16) is None, text
    assert geotags.stored_nodata(GEO[:3], 16) is None and geotags.stored_nodata(None, 16) is None


# ---------------------------------------------------------------- read_geo_tags touches no pixel

class Recorder:
    """a file as len() and slices, noting every byte range asked of it"""

    def __init__(self, data):
        self.data, self.asked, self.closed = data, [], False

    def __len__(self):
        return len(self.data)

    def __getitem__(self, key):
        assert isinstance(key, slice) and key.step in (None, 1)
        a, b, _ = key.indices(len(self.data))
        self.asked.append((a, b))
        return self.data[a:b]

    def close(self):
        self.closed = True


@pytest.mark.parametrize("layout", ("strips", "tiles", "bigendian"))
def test_read_geo_tags_reads_the_header_the_ifd_and_the_values_only(layout, tmp_path, monkeypatch):
    from lbdrn_hip import raster_io, tiff
    a = np.random.default_rng(2).integers(0, 60000, (3, 40, 48)).astype(np.uint16)
    kw = {"strips": dict(rows_per_strip=7), "tiles": dict(tile=(16, 16), compression=TR.COMP_DEFLATE, predictor=2),
          "bigendian": dict(byteorder=">")}[layout]
    plain, info = TR.write_tiff(a, **kw)
    data = with_tags(plain, GEO)
    today = tiff.read_geo_tags(data)
    assert today == GEO and tiff.read_geo_tags(plain) == []
    rec = Recorder(data)
    assert tiff.read_geo_tags(rec) == today
    segments = list(zip(info["offsets"], info["counts"]))
    assert len(segments) >= 3 and sum(c for _, c in segments) > len(data) // 2
    touched = lambda rec: [(lo, hi, o, c) for lo, hi in rec.asked for o, c in segments if lo < o + c and o < hi]
    assert rec.asked and not touched(rec)
    assert sum(hi - lo for lo, hi in rec.asked) < 1200
    # raster_io goes through the memory map and gives it back
    path = str(tmp_path / "scene.tif")
    with open(path, "wb") as f:
        f.write(data)
    maps = []
    monkeypatch.setattr(tiff, "open_map", lambda p: maps.append(Recorder(open(p, "rb").read())) or maps[-1])
    assert raster_io.read_geo_tags(path) == today
    assert len(maps) == 1 and maps[0].closed and maps[0].asked and not touched(maps[0])
    monkeypatch.undo()
    assert raster_io.read_geo_tags(path) == today and raster_io.read_geo_tags(str(tmp_path / "x.npy")) == []


# ---------------------------------------------------------------- encode.py / sweep.py --keep-tags with stand-ins

ARGS = ["-sr", "3", "-K", "4", "-e", "2", "-bs", "64"]
SUB = "scene_r3_K4_bc64_nl2_D2_prec16_lr0.001_bs64_e2"
IMG = np.random.default_rng(4).integers(0, 9000, (2, 31, 40)).astype(np.uint16)
SCENE_TAGS = [GEO[0], GEO[1]] + GEO[3:]      # (a pixel scale and one tiepoint: the form a crop moves by the scale)


def _scene(path, img=IMG, tags=SCENE_TAGS):
    data = TR.write_tiff(img, rows_per_strip=5)[0]
    with open(path, "wb") as f:
        f.write(with_tags(data, tags) if tags else data)
    return str(path)


def _stand_ins(monkeypatch):
    import encode
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    monkeypatch.setattr(encode, "residual_layer", _stub_layer)
    monkeypatch.setattr(encode, "BASE_CODEC", "LBB2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBDRN_TILE_READS"):
        monkeypatch.delenv(k, raising=False)
    return encode


def _encode_worker(rank, world, port, src, out_dir, extra):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import encode
    encode.train_tiles, encode.report_and_pack, encode.residual_layer = _stub_train_tiles, _stub_report, _stub_layer
    if rank != 0:      # only rank 0 opens the tags

        def never(path):
            raise AssertionError(f"rank {rank} read the tags of {path}")
        encode.raster_io.read_geo_tags = never
    assert encode.main(["-i", src, "-o", out_dir] + ARGS + extra) == 0


def test_keep_tags_appends_the_chunk_and_nothing_else_changes(tmp_path, monkeypatch):
    from lbdrn_hip import container, geotags
    encode = _stand_ins(monkeypatch)
    (tmp_path / "tagged").mkdir()
    (tmp_path / "bare").mkdir()
    src, bare = _scene(tmp_path / "tagged" / "scene.tif"), _scene(tmp_path / "bare" / "scene.tif", tags=None)
    npy = str(tmp_path / "scene.npy")
    np.save(npy, IMG)
    run = lambda name, path, extra: (encode.main(["-i", path, "-o", str(tmp_path / name)] + ARGS + extra),
                                     (tmp_path / name / SUB / "scene.bin").read_bytes(), _records(tmp_path / name / SUB / "encode.txt"))[1:]
    plain, recs_plain = run("plain", src, [])
    kept, recs_kept = run("kept", src, ["--keep-tags"])
    chunk = container.pack_geo_trailer(SCENE_TAGS)
    assert kept == plain + chunk and container.unpack_geo_trailer(kept) == SCENE_TAGS and container.unpack_geo_trailer(plain) is None
    assert len(plain) == container.residual_trailer_offset(kept)
    # without the flag the tags of the input do not matter; nor does the kind of file
    assert run("bare", bare, [])[0] == plain == run("npy", npy, [])[0]
    # a source without tags: no chunk, and a record that says so
    for name, path in (("bare-kept", bare), ("npy-kept", npy)):
        data, recs = run(name, path, ["--keep-tags"])
        assert data == plain and recs[-2] == "Tags: none" and recs[-1].startswith("Time elapsed: ")
    # the records: one more, in front of `Time elapsed`, and none of results_summary.py's patterns matches it
    assert recs_kept[-2] == f"Tags: {len(SCENE_TAGS)} tags, {len(chunk)} bytes" and recs_kept[-1].startswith("Time elapsed: ")
    assert not any(r.startswith("Tags") for r in recs_plain)
    same = lambda recs, name: [r.replace(str(tmp_path / name), "X") for r in recs if not r.startswith(("Time elapsed", "Tags", "Namespace"))]
    assert same(recs_kept, "kept") == same(recs_plain, "plain")
    import results_summary as R
    for pattern in [p for p, _ in R.DECODE_RECORDS.values()] + [R.ELAPSED] + list(R.ENCODE_RECORDS.values()):
        assert pattern.search(recs_kept[-2]) is None and pattern.search("Tags: none") is None
    assert R.extract_metrics1(str(tmp_path / "kept" / SUB / "encode.txt")) == R.extract_metrics1(str(tmp_path / "plain" / SUB / "encode.txt"))
    # two gloo ranks: the serial file; ranks other than 0 never open the tags
    mp.spawn(_encode_worker, args=(2, 29100 + os.getpid() % 150, src, str(tmp_path / "sharded"), ["--keep-tags"]), nprocs=2, join=True)
    assert (tmp_path / "sharded" / SUB / "scene.bin").read_bytes() == kept
    strip = lambda recs, name: [r.replace(str(tmp_path / name), "X") for r in recs if not r.startswith("Time elapsed")]
    assert strip(_records(tmp_path / "sharded" / SUB / "encode.txt"), "sharded") == strip(recs_kept, "kept")
    # --max-error with --keep-tags: both trailers, the layer's first
    layered = run("layer", src, ["--max-error", "3"])[0]
    both = run("layer-kept", src, ["--max-error", "3", "--keep-tags"])[0]
    assert both == layered + chunk and layered[:len(plain)] == plain
    assert container.unpack_residual_trailer(both) == container.unpack_residual_trailer(layered) != None      # noqa: E711
    assert container.unpack_geo_trailer(both) == SCENE_TAGS and container.unpack_geo_trailer(layered) is None
    mp.spawn(_encode_worker, args=(2, 29260 + os.getpid() % 150, src, str(tmp_path / "sharded-layer"), ["--max-error", "3", "--keep-tags"]),
             nprocs=2, join=True)
    assert (tmp_path / "sharded-layer" / SUB / "scene.bin").read_bytes() == both
    assert geotags.shift(SCENE_TAGS, 0, 0) == SCENE_TAGS


def test_keep_tags_under_a_window_stores_the_tags_of_the_crop(tmp_path, monkeypatch):
    from lbdrn_hip import container, geotags
    encode = _stand_ins(monkeypatch)
    x0, y0, w, h = 7, 5, 26, 21
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    src = _scene(tmp_path / "a" / "scene.tif")
    moved = geotags.shift(SCENE_TAGS, x0, y0)
    assert moved != SCENE_TAGS and doubles(_tag(moved, 33922)[3])[3:5] == (399960.0 + 70.0, 5700000.5 - 50.0)
    crop = _scene(tmp_path / "b" / "scene.tif", img=np.ascontiguousarray(IMG[:, y0:y0 + h, x0:x0 + w]), tags=moved)
    assert encode.main(["-i", src, "-o", str(tmp_path / "win"), "--window", str(x0), str(y0), str(w), str(h), "--keep-tags"] + ARGS) == 0
    assert encode.main(["-i", crop, "-o", str(tmp_path / "crop"), "--keep-tags"] + ARGS) == 0
    got = (tmp_path / "win" / SUB.replace("scene", f"scene_x{x0}_y{y0}_w{w}_h{h}") / f"scene_x{x0}_y{y0}_w{w}_h{h}.bin").read_bytes()
    assert got == (tmp_path / "crop" / SUB / "scene.bin").read_bytes()
    assert container.unpack_geo_trailer(got) == moved and got.endswith(container.pack_geo_trailer(moved))
    # LBDRN_TILE_READS: the same file
    monkeypatch.setenv("LBDRN_TILE_READS", "1")
    assert encode.main(["-i", src, "-o", str(tmp_path / "win-reads"), "--window", str(x0), str(y0), str(w), str(h), "--keep-tags"] + ARGS) == 0
    assert got == (tmp_path / "win-reads" / SUB.replace("scene", f"scene_x{x0}_y{y0}_w{w}_h{h}") / f"scene_x{x0}_y{y0}_w{w}_h{h}.bin").read_bytes()


def test_main_k_points_and_the_sweep_put_the_chunk_in_every_file(tmp_path, monkeypatch):
    import sweep
    from lbdrn_hip import container
    encode = _stand_ins(monkeypatch)
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles_k)
    monkeypatch.setattr(encode, "train_tiles_at", _stub_train_tiles_at)
    monkeypatch.setattr(sweep.decode, "main", lambda argv, shard_tiles=None: 0)
    src = _scene(tmp_path / "scene.tif")
    chunk = container.pack_geo_trailer(SCENE_TAGS)
    common = ["-sr", "3", "-e", "2", "-bs", "64"]
    Ks = (3, 4, 5)
    sub = lambda K: f"scene_r3_K{K}_bc64_nl2_D2_prec16_lr0.001_bs64_e2"
    for K in Ks:
        assert encode.main(["-i", src, "-o", str(tmp_path / "one"), "-K", str(K)] + common, shard_tiles=False) == 0
    for extra in ([], ["--max-error", "3"]):
        tag = "layer" if extra else "plain"
        for K in Ks:
            assert encode.main(["-i", src, "-o", str(tmp_path / f"one-{tag}"), "-K", str(K), "--keep-tags"] + common + extra, shard_tiles=False) == 0
        assert encode.main_k_points(["-i", src, "-o", str(tmp_path / f"many-{tag}"), "--keep-tags"] + common + extra, Ks) == {K: None for K in Ks}
        for K in Ks:
            a, b = ((tmp_path / f"{d_}-{tag}" / sub(K) / "scene.bin").read_bytes() for d_ in ("one", "many"))
            assert a == b and a.endswith(chunk) and container.unpack_geo_trailer(b) == SCENE_TAGS
            assert (container.unpack_residual_trailer(b) is not None) == bool(extra)
            if not extra:
                assert a == (tmp_path / "one" / sub(K) / "scene.bin").read_bytes() + chunk
            recs = _records(tmp_path / f"many-{tag}" / sub(K) / "encode.txt")
            assert recs[-2] == f"Tags: {len(SCENE_TAGS)} tags, {len(chunk)} bytes" and recs[-1].startswith("Time elapsed: ")
    # sweep.py passes the flag on, point after point and with the K points side by side; without it, today's files
    for name, extra in (("sweep", ["--keep-tags"]), ("sweep-k", ["--keep-tags", "--k-in-flight", "2"]), ("sweep-bare", [])):
        argv = ["--images", src, "--k", "3", "5", "-o", str(tmp_path / name), "-sr", "3", "-e", "2", "-bs", "64"] + extra
        assert ("--keep-tags" in sweep.common_args(sweep.parse(argv))) == ("--keep-tags" in extra)
        assert sweep.main(argv) == 0
        for K in Ks:
            want = (tmp_path / "one" / sub(K) / "scene.bin").read_bytes() + (chunk if extra else b"")
            assert (tmp_path / name / sub(K) / "scene.bin").read_bytes() == want, (name, K)


def test_run_sh_reads_keep_tags(tmp_path):
    """KEEP_TAGS=1 ./run.sh ... hands --keep-tags to sweep.py; without the variable, and with KEEP_TAGS=0, today's command line
    (`python` is a stand-in that prints its arguments)"""
    fake = tmp_path / "python"
    fake.write_text('#!/bin/bash\nprintf "%s\\n" "$@"\n')
    fake.chmod(0o755)
    positional = ["0", "2", "64", "2", "0.001", "8192", "10", "1", "outputs"]
    env = {k: v for k, v in os.environ.items() if k not in ("NGPU", "K_IN_FLIGHT", "PER_GPU", "KEEP_TAGS")}
    env.update(PATH=f"{tmp_path}:{env['PATH']}", PER_GPU="1")
    run = lambda e: subprocess.run(["bash", os.path.join(PKG, "run.sh")] + positional, env=e, capture_output=True, text=True,
                                   check=True).stdout.split("\n")[:-1]
    plain = run(env)
    assert plain == [os.path.join(PKG, "sweep.py")] + positional == run(dict(env, KEEP_TAGS="0"))
    got = run(dict(env, KEEP_TAGS="1", K_IN_FLIGHT="2"))
    assert got == plain + ["--k-in-flight", "2", "--keep-tags"]
    import sweep
    assert sweep.parse(got[1:]).keep_tags and not sweep.parse(plain[1:]).keep_tags


# ---------------------------------------------------------------- python -m lbdrn_hip.geotags

def test_attach_gives_what_keep_tags_writes_and_strip_gives_it_back(tmp_path, monkeypatch, capsys):
    from lbdrn_hip import container, geotags
    encode = _stand_ins(monkeypatch)
    src = _scene(tmp_path / "scene.tif")
    x0, y0, w, h = 7, 5, 26, 21
    win = ["--window", str(x0), str(y0), str(w), str(h)]
    stem = f"scene_x{x0}_y{y0}_w{w}_h{h}"
    cases = {"plain": ([], SUB, "scene"), "layer": (["--max-error", "3"], SUB, "scene"), "window": (win, SUB.replace("scene", stem), stem)}
    for name, (extra, sub, binname) in cases.items():
        assert encode.main(["-i", src, "-o", str(tmp_path / name)] + ARGS + extra) == 0
        assert encode.main(["-i", src, "-o", str(tmp_path / (name + "-kept")), "--keep-tags"] + ARGS + extra) == 0
        bare = tmp_path / name / sub / f"{binname}.bin"
        kept = (tmp_path / (name + "-kept") / sub / f"{binname}.bin").read_bytes()
        original = bare.read_bytes()
        out = str(tmp_path / f"{name}-attached.bin")
        assert geotags._cli(["--attach", src, str(bare), "-o", out] + (win if name == "window" else [])) == 0
        assert open(out, "rb").read() == kept and bare.read_bytes() == original
        with pytest.raises(SystemExit):      # a file that already has one
            geotags._cli(["--attach", src, out])
        assert open(out, "rb").read() == kept
        back = str(tmp_path / f"{name}-stripped.bin")
        assert geotags._cli(["--strip", out, "-o", back]) == 0
        assert open(back, "rb").read() == original
        assert geotags._cli(["--strip", out]) == 0 and open(out, "rb").read() == original      # in place
        assert geotags._cli(["--strip", out]) == 0 and open(out, "rb").read() == original      # nothing to remove: as it is
        assert geotags._cli(["--attach", src, out] + (win if name == "window" else [])) == 0 and open(out, "rb").read() == kept
        assert (container.unpack_residual_trailer(kept) is not None) == (name == "layer")
    with pytest.raises(SystemExit):          # the scene's size against a file that holds a window of it
        geotags._cli(["--attach", src, str(tmp_path / "window" / cases["window"][1] / f"{stem}.bin")])
    capsys.readouterr()
    # printing: the module as a program, on the .bin and on the TIFF
    kept = str(tmp_path / "plain-kept" / SUB / "scene.bin")
    run = lambda path: subprocess.run([sys.executable, "-m", "lbdrn_hip.geotags", path], cwd=PKG, capture_output=True, text=True, check=True).stdout
    lines = run(kept).splitlines()
    assert lines == run(src).splitlines() == geotags.describe(SCENE_TAGS) and len(lines) == len(SCENE_TAGS)
    assert lines[1] == "33922 ModelTiepoint (6): 0.0 0.0 0.0 399960.0 5700000.5 0.0" and lines[-1] == "42113 GDAL_NODATA (2): '0'"
    assert geotags._cli([str(tmp_path / "plain" / SUB / "scene.bin")]) == 0 and capsys.readouterr().out == "no tags\n"


# ---------------------------------------------------------------- decode.py with stand-ins: who gets the tags

def test_decode_hands_the_stored_tags_to_the_writer(tmp_path, monkeypatch):
    """A whole decode at -sr 2 with the device work and the writer replaced by stand-ins: the merged raster is written with the
    stored tags, with none under --no-tags and for a file without the chunk, and the residual trailer in front of the chunk is
    still found.  (The window's move and every real writer path: tests/test_gpu_geotags.py.)"""
    import decode
    from lbdrn_hip import codec, container, raster_io
    from test_cli_sharding_cpu import _stub_apply
    nn, base = [b"w" * 10] * 4, [bytes(range(t, t + 48)) + b"pad" * t for t in range(4)]
    blob = container.pack_header(2, 12, 8, 3, 64, 2, 2, [len(x) for x in nn], [len(x) for x in base])
    blob += b"".join(x + y for x, y in zip(nn, base))
    chunk = container.pack_geo_trailer(SCENE_TAGS)
    monkeypatch.setattr(codec, "apply_image", _stub_apply)
    monkeypatch.setattr(container, "decode_weights", lambda payload, expected=None: np.zeros(4, np.float32))
    monkeypatch.setattr(container, "decode_base",
                        lambda payload, device=None, keep_on_device=False: np.frombuffer(payload[:48], np.uint8).reshape(2, 4, 6).copy())
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    written, plain_write = [], raster_io.write_raster

    def write_raster(path, array, **kw):
        written.append((os.path.basename(os.path.dirname(path)), kw.get("geo")))
        plain_write(path, array)
    monkeypatch.setattr(raster_io, "write_raster", write_raster)
    outs = {}
    for name, data, flags in (("bare", blob, []), ("kept", blob + chunk, []), ("ignored", blob + chunk, ["--no-tags"]),
                              ("base-only", blob + chunk, ["--no-enhancement"])):
        d_ = tmp_path / name
        d_.mkdir()
        (d_ / "img.bin").write_bytes(data)
        assert decode.main(["-i", str(d_ / "img.bin")] + flags) == 0
        outs[name] = ((d_ / "img_recon.tif").read_bytes(), [r.split(":")[0] for r in _records(d_ / "decode.txt")])
    assert written == [("bare", None), ("kept", SCENE_TAGS), ("ignored", None), ("base-only", SCENE_TAGS)]
    assert outs["bare"][1] == outs["ignored"][1] == ["Binstream", "Time elapsed"]
    assert outs["kept"][1] == outs["base-only"][1] == ["Binstream", "Tags", "Time elapsed"]
    assert _records(tmp_path / "kept" / "decode.txt")[1] == f"Tags: {len(SCENE_TAGS)} tags restored"
    assert outs["bare"][0] == outs["ignored"][0]
    # a damaged chunk, or a byte behind it, stops the decode before anything is written
    for k, bad in enumerate((blob + chunk[:-1], blob + chunk + b"\0", blob + chunk + chunk)):
        d_ = tmp_path / f"bad{k}"
        d_.mkdir()
        (d_ / "img.bin").write_bytes(bad)
        with pytest.raises(ValueError):
            decode.main(["-i", str(d_ / "img.bin")])
        assert not (d_ / "img_recon.tif").exists()
