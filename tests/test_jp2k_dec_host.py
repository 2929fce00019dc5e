"""The GPU JPEG 2000 decoder's host-compilable text (csrc/jp2k_t1d.inc: the tier-1 decoder the kernel runs; csrc/jp2k_t2d.inc:
boxes, headers, geometry, packet headers, the validated block table) judged on the CPU against the oracle
(oracle/jp2k_oracle.c), through tests/jp2k_dec_host_shim.cpp compiled by g++ into a temporary directory -- and the host
logic around the decoder: lbdrn_jp2kd_info without a device, the reader container.decode_base chooses, the exports and
the kernels' resources of liblbdrn_jp2k_dec.so.  No GPU.  Every comparison is exact.

Inputs the product reads are handed over in memory that ENDS at an inaccessible page (GuardedBytes): a read behind the
buffer is a fault, not a silent success.  tests/test_gpu_jp2k_dec.py imports the helpers and the damaged-file lists."""
import ctypes
import mmap
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import jp2k as oracle  # noqa: E402
from test_jp2k_host import GEOMETRIES  # noqa: E402
from test_jp2k_oracle import NEW_GEOMETRIES, fuzz_blocks, planes_of, random_packet  # noqa: E402

F = oracle.F
CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
DEC_LIB = os.path.join(ROOT, "lbdrn-msic_amd", "liblbdrn_jp2k_dec.so")
DEC_BAD, DEC_UNSUPPORTED = -1, -3
_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
_shim = None


def build_shim(out_dir):
    """g++ -> libjp2k_dec_host_shim.so in out_dir.  LBDRN_JP2K_DEC_SHIM_SANITIZE=1 (scripts/sanitize_jp2k_dec.sh) adds
    AddressSanitizer and UndefinedBehaviorSanitizer."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        return None
    assert os.path.exists(os.path.join(CSRC, "jp2k_t1d.inc")) and os.path.exists(os.path.join(CSRC, "jp2k_t2d.inc")), \
        "csrc/jp2k_t1d.inc and csrc/jp2k_t2d.inc (the decoder's host-compilable text) do not exist"
    out = os.path.join(str(out_dir), "libjp2k_dec_host_shim.so")
    opt = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] \
        if os.environ.get("LBDRN_JP2K_DEC_SHIM_SANITIZE") == "1" else ["-O2"]
    subprocess.check_call([cxx] + opt + ["-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                                         os.path.join(ROOT, "tests", "jp2k_dec_host_shim.cpp")])
    return out


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        path = build_shim(tmp_path_factory.mktemp("jp2k_dec_shim"))
        if path is None:
            pytest.skip("no host C++ compiler (g++): the decoder's host text cannot be compiled")
        L = ctypes.CDLL(path)
        L.jp2kd_shim_t1_decode.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _i]
        L.jp2kd_shim_packet_header.argtypes = [_i, _vp, _vp, _vp, _vp, _sz, _vp]
        L.jp2kd_shim_packet_header.restype = _i64
        L.jp2kd_shim_info.argtypes = [_vp, _sz, _vp, _vp, _sz]
        L.jp2kd_shim_parse.argtypes = [_vp, _sz, _vp, _i64, _vp, _sz]
        L.jp2kd_shim_parse.restype = _i64
        _shim = L
    return _shim


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


class GuardedBytes:
    """room for `cap` bytes that ends exactly where an inaccessible page begins; put(data) places data against it"""

    def __init__(self, cap):
        page = mmap.PAGESIZE
        self.cap = max(int(cap), 1)
        self.size = (self.cap + page - 1) // page * page + page
        self.m = mmap.mmap(-1, self.size)
        self.anchor = ctypes.c_char.from_buffer(self.m)
        self.base = ctypes.addressof(self.anchor)
        libc = ctypes.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [_vp, _sz, _i]
        assert libc.mprotect(_vp(self.base + self.size - page), page, 0) == 0, os.strerror(ctypes.get_errno())   # PROT_NONE
        self.end = self.size - page

    def put(self, data):
        data = bytes(data)
        assert len(data) <= self.cap
        start = self.end - len(data)
        self.m[start:self.end] = data
        return _vp(self.base + start), len(data)


def _p(a):
    return a.ctypes.data_as(_vp)


def shim_t1_decode(L, room, data, w, h, orient, numbps, passes, canary=97):
    """the product's block decoder on `data` (placed against the guard page of `room`) -> [h, w] int32; asserts the canary
    behind and between the rows of the output"""
    ptr, n = room.put(data)
    stride = w + 3
    out = np.full(h * stride + canary, -0x5A5A5A5B, np.int32)
    assert L.jp2kd_shim_t1_decode(ptr, n, w, h, orient, numbps, passes, _p(out), stride) == 0
    body = out[:h * stride].reshape(h, stride)
    assert (out[h * stride:] == -0x5A5A5A5B).all() and (body[:, w:] == -0x5A5A5A5B).all(), "the block decoder wrote outside its block"
    return np.ascontiguousarray(body[:, :w])


def shim_info(L, buf, room=None):
    """-> (code, dict or message)"""
    room = room or GuardedBytes(len(buf))
    ptr, n = room.put(buf)
    out = np.zeros(9, np.int64)
    msg = ctypes.create_string_buffer(300)
    rc = L.jp2kd_shim_info(ptr, n, _p(out), msg, 300)
    if rc:
        return rc, msg.value.decode(errors="replace")
    return 0, dict(zip(("C", "H", "W", "bits", "tiles", "blocks", "resolutions", "tw", "th"), (int(v) for v in out)))


def shim_parse(L, buf, room=None, cap=1 << 14):
    """-> (code, message) or (0, int64 [n, 16] in the columns of oracle.FIELDS)"""
    room = room or GuardedBytes(len(buf))
    ptr, n = room.put(buf)
    msg = ctypes.create_string_buffer(300)
    while True:
        rec = np.zeros((cap, 16), np.int64)
        got = L.jp2kd_shim_parse(ptr, n, _p(rec), cap, msg, 300)
        if got < 0:
            return int(got), msg.value.decode(errors="replace")
        if got <= cap:
            return 0, rec[:got]
        cap = int(got)      # (a damaged header may announce more blocks than the room that was offered)


def table_is_valid(rec, n):
    """what the device relies on (the head of csrc/jp2k_t2d.inc), per block"""
    inc = rec[rec[:, F["passes"]] > 0]
    ok = (rec[:, F["w"]] >= 1).all() and (rec[:, F["w"]] <= 64).all() and (rec[:, F["h"]] >= 1).all() and (rec[:, F["h"]] <= 64).all()
    ok = ok and (rec[:, F["passes"]] >= 0).all()
    ok = ok and (inc[:, F["offset"]] >= 0).all() and (inc[:, F["length"]] >= 0).all() and (inc[:, F["offset"]] + inc[:, F["length"]] <= n).all()
    ok = ok and (inc[:, F["numbps"]] >= 1).all() and (inc[:, F["numbps"]] <= inc[:, F["mb"]]).all() and (inc[:, F["mb"]] <= 31).all()
    ok = ok and (inc[:, F["passes"]] <= 3 * inc[:, F["numbps"]] - 2).all()
    return bool(ok)


# ------------------------------------------------------------------ tier-1

def test_block_decoder_inverts_the_oracle_coder_and_equals_the_oracle_decoder_at_every_pass_count(shim):
    """The 520-block fuzz of tests/test_jp2k_oracle.py: from oracle.t1_encode's bytes the product's decoder reads exactly
    the coefficients that went in, and for every pass count from 1 to the full count what oracle.t1_decode reads."""
    oracle.counters(reset=True)
    room = GuardedBytes(1 << 16)
    blocks = seen = 0
    for w, h, orient, numbps, stat, a in fuzz_blocks(20261016):
        data, passes, nb = oracle.t1_encode(a, orient)
        blocks += 1
        where = f"tier-1 block decoder (jp2k_t1d.inc): {w} x {h}, orientation {orient}, numbps {numbps}, {stat}"
        if stat == "zero":
            assert (passes, nb) == (0, 0)
            assert not shim_t1_decode(shim, room, b"", w, h, orient, 0, 0).any(), where
            continue
        assert (nb, passes) == (numbps, 3 * numbps - 2), where
        got = shim_t1_decode(shim, room, data, w, h, orient, nb, passes)
        assert np.array_equal(got, a), f"{where}: {int((got != a).sum())} coefficients differ, first at {tuple(np.argwhere(got != a)[0])}"
        for k in range(1, passes + 1):
            want = oracle.t1_decode(data, w, h, orient, nb, k)
            got = shim_t1_decode(shim, room, data, w, h, orient, nb, k)
            assert np.array_equal(got, want), f"{where}: after {k} of {passes} passes {int((got != want).sum())} coefficients differ from the oracle's"
        seen += 1
    assert blocks == 520 and seen >= 470
    c = oracle.counters()
    for name in ("rl_exit0", "rl_exit1", "rl_exit2", "rl_exit3", "rl_zero", "partial_stripe", "narrow_block"):
        assert c[name] > 0, (name, c)


def test_block_decoder_terminates_on_every_prefix_and_stays_inside_its_block(shim):
    """Every prefix of a block's bytes -- each placed against an inaccessible page, so that a read behind it faults --
    decodes to something in bounded time, with the canaries around the output intact.  Literally every prefix for the
    blocks of the fuzz whose segment has at most 512 bytes (a decode costs w * h * planes decisions whatever the length,
    so every prefix of the 9 KB segments would cost minutes); of the longer ones the first and last 64 prefixes and 64
    evenly spaced ones between.  The full segment gives the block back; a prefix agrees with the oracle's decoder, which
    is fed the same 0xFF fill behind the data."""
    room = GuardedBytes(1 << 16)
    n_all = n_some = 0
    for w, h, orient, numbps, stat, a in fuzz_blocks(20261016):
        if stat == "zero":
            continue
        data, passes, nb = oracle.t1_encode(a, orient)
        if len(data) <= 512:
            cuts = range(len(data) + 1)
            n_all += 1
        else:
            cuts = sorted(set(range(64)) | set(range(len(data) - 63, len(data) + 1)) | set(np.linspace(64, len(data) - 64, 64).astype(int).tolist()))
            n_some += 1
        for cut in cuts:
            got = shim_t1_decode(shim, room, data[:cut], w, h, orient, nb, passes)
            if cut == len(data):
                assert np.array_equal(got, a)
            elif cut % 7 == 0:
                assert np.array_equal(got, oracle.t1_decode(data[:cut], w, h, orient, nb, passes)), (w, h, orient, numbps, stat, cut)
    assert n_all + n_some == 480 and n_all > 0 and n_some > 0, (n_all, n_some)      # every non-zero block of the fuzz


# ------------------------------------------------------------------ tier-2

def test_packet_header_parser_equals_the_oracle_parser(shim):
    rng = np.random.default_rng(410)
    room = GuardedBytes(1 << 16)
    for k in range(400):
        gw, gh, mb, rec = random_packet(rng, k)
        data = oracle.packet_header_write(gw, gh, mb, rec) + b"\x12\x34"
        want, used = oracle.packet_header_parse(gw, gh, mb, data)
        gwa, gha, mba = (np.ascontiguousarray(v, dtype=np.int32) for v in (gw, gh, mb))
        got = np.full((max(len(rec), 1) + 1, 3), -77, np.int32)
        ptr, n = room.put(data)
        m = shim.jp2kd_shim_packet_header(len(gw), _p(gwa), _p(gha), _p(mba), ptr, n, _p(got))
        where = f"tier-2 packet header (jp2k_t2d.inc dec_packet_header): packet {k}, grids {list(zip(gw, gh))}"
        assert m == used == len(data) - 2, f"{where}: header of {m} bytes, the oracle reads {used}"
        assert np.array_equal(got[:len(rec)], want) and np.array_equal(want, rec), f"{where}: other records than the oracle's"
        assert (got[len(rec):] == -77).all() or len(rec) == 0, f"{where}: records behind the packet's blocks were written"
        # cut short, the header is an error, not a read behind the data
        for cut in {0, 1, max(used - 1, 0)}:
            ptr, n = room.put(data[:cut])
            r = shim.jp2kd_shim_packet_header(len(gw), _p(gwa), _p(gha), _p(mba), ptr, n, _p(got))
            assert r <= cut


def whole_file_cases():
    for H, W in GEOMETRIES + NEW_GEOMETRIES:
        if H * W <= 1100 * 1100:
            yield f"oracle {H} x {W}", oracle.encode(planes_of("synth", (2 if H * W < 300000 else 1, H, W), 16))
        else:      # the large geometries as empty planes: every block of the geometry, every packet empty
            yield f"oracle {H} x {W} (mid-grey)", oracle.encode(np.full((1, H, W), 128, np.uint8))


def assert_table_equals_oracle(L, name, f):
    want = oracle.parse(f)
    rc, got = shim_parse(L, f, cap=len(want) + 8)
    assert rc == 0, f"{name}: the product's parser answers {rc}: {got}"
    assert got.shape == want.shape, f"{name}: {len(got)} blocks, the oracle has {len(want)}"
    for field in oracle.FIELDS:
        bad = np.nonzero(got[:, F[field]] != want[:, F[field]])[0]
        assert not len(bad), (f"{name}: block {bad[0]} (tile {want[bad[0], 0]}, comp {want[bad[0], 1]}, res {want[bad[0], 2]}): {field} is "
                              f"{got[bad[0], F[field]]}, the oracle has {want[bad[0], F[field]]}")
    assert table_is_valid(got, len(f)), name
    rc, i = shim_info(L, f)
    oi = oracle.info(f)
    assert rc == 0 and all(i[k] == oi[k] for k in ("C", "H", "W", "bits", "tiles", "blocks", "resolutions")), (name, i, oi)


def test_block_table_equals_the_oracle_parse_on_the_oracles_files(shim):
    n = 0
    for name, f in whole_file_cases():
        assert_table_equals_oracle(shim, name, f)
        n += 1
    assert n == 30
    for stat, bits in (("uniform", 16), ("sparse", 16), ("spike", 8), ("checker", 8), ("zero", 16)):
        assert_table_equals_oracle(shim, f"oracle 3 x 130 x 1030 {stat}", oracle.encode(planes_of(stat, (3, 130, 1030), bits)))


def test_block_table_equals_the_oracle_parse_on_every_openjpeg_file_of_the_fixture(shim, golden):
    g = golden["jp2k_openjpeg"]
    names = sorted(k[len("file_"):] for k in g.files if k.startswith("file_"))
    assert len(names) >= 6
    for name in names:
        f = g["file_" + name].tobytes()
        rc, i = shim_info(shim, f)
        assert rc == 0, f"fixture file {name}: refused with {rc}: {i}"
        assert (i["C"], i["H"], i["W"]) == g["planes_" + name].shape
        assert_table_equals_oracle(shim, f"fixture file {name}", f)


def with_tile_parts_split(f):
    """the oracle's one-tile file rewritten with its packets in two tile-parts (Psot = 0 in the second), a COM segment in
    the main header and one in the second tile-part's header: same packets, other framing"""
    rec = oracle.parse(f)
    at = f.index(b"jp2c") + 4
    sot = f.index(b"\xff\x90", at)
    assert oracle.info(f)["tiles"] == 1 and f[sot + 12:sot + 14] == b"\xff\x93" and f[-2:] == b"\xff\xd9"
    # a packet boundary in the middle: where the first block of the second resolution's first packet begins, minus its header
    inc = rec[(rec[:, F["passes"]] > 0) & (rec[:, F["res"]] == 0)]
    cut = int((inc[:, F["offset"]] + inc[:, F["length"]]).max())        # the end of resolution 0's last packet
    com = b"\xff\x64" + (2 + 2 + 5).to_bytes(2, "big") + b"\x00\x01hello"
    part1 = f[sot + 14:cut]
    part2 = f[cut:-2]
    p1 = b"\xff\x90\x00\x0a\x00\x00" + (14 + len(part1)).to_bytes(4, "big") + b"\x00\x02" + b"\xff\x93" + part1
    p2 = b"\xff\x90\x00\x0a\x00\x00" + (0).to_bytes(4, "big") + b"\x01\x02" + com + b"\xff\x93" + part2
    stream = f[at:sot] + com + p1 + p2 + b"\xff\xd9"
    return f[:at - 8] + (8 + len(stream)).to_bytes(4, "big") + b"jp2c" + stream


def test_tile_parts_com_segments_raw_codestreams_and_unsupported_features(shim):
    x = planes_of("synth", (1, 1, 1), 16)
    f = oracle.encode(planes_of("synth", (2, 90, 130), 16))
    want = oracle.parse(f)
    # two tile-parts, Psot = 0 in the last, COM in both headers: the same blocks at shifted offsets
    g = with_tile_parts_split(f)
    rc, got = shim_parse(shim, g)
    assert rc == 0, got
    cols = [F[k] for k in oracle.FIELDS if k != "offset"]
    assert np.array_equal(got[:, cols], want[:, cols])
    for a, b in zip(got, want):
        if b[F["passes"]]:
            assert g[a[F["offset"]]:a[F["offset"]] + a[F["length"]]] == f[b[F["offset"]]:b[F["offset"]] + b[F["length"]]]
    # the raw codestream without its boxes
    at = f.index(b"jp2c") + 4
    rc, got = shim_parse(shim, f[at:])
    assert rc == 0 and np.array_equal(got[:, cols], want[:, cols])
    # what the decoder does not take is named, before anything else happens
    del x
    cod = f.index(b"\xff\x52", at)
    siz = f.index(b"\xff\x51", at)
    qcd = f.index(b"\xff\x5c", at)

    def patched(pos, value):
        b = bytearray(f)
        b[pos] = value
        return bytes(b)
    for what, data, word in (("9/7", patched(cod + 13, 0), "9/7"), ("two layers", patched(cod + 7, 2), "layers"),
                             ("RLCP", patched(cod + 5, 1), "progression"), ("bypass style", patched(cod + 12, 1), "style"),
                             ("explicit precincts", patched(cod + 4, 1), "precinct"), ("component transform", patched(cod + 8, 1), "component transform"),
                             ("128-wide code blocks", patched(cod + 10, 5), "code blocks"), ("signed", patched(siz + 40, 0x8F), "signed"),
                             ("sub-sampled", patched(siz + 41, 2), "sub-sampled"), ("quantised", patched(qcd + 4, 0x42), "quantisation")):
        rc, msg = shim_info(shim, data)
        assert rc == DEC_UNSUPPORTED and word in msg, (what, rc, msg)
    for marker, word in ((b"\xff\x60", "PPM"), (b"\xff\x53", "COC"), (b"\xff\x5f", "POC")):
        data = f[:cod] + marker + b"\x00\x04\x00\x00" + f[cod:]
        data = data[:at - 8] + (len(data) - at + 8).to_bytes(4, "big") + data[at - 4:]
        rc, msg = shim_info(shim, data)
        assert rc == DEC_UNSUPPORTED and word in msg, (marker.hex(), rc, msg)
    rc, msg = shim_info(shim, b"\x00\x00\x00\x0cjP  \r\n\x87\n" + b"\x00" * 40)
    assert rc == DEC_BAD and msg


# ------------------------------------------------------------------ robustness

def small_files(golden):
    """two small files: the oracle's (two components, several packets per resolution) and the smallest of the fixture"""
    g = golden["jp2k_openjpeg"]
    names = sorted((k for k in g.files if k.startswith("file_")), key=lambda k: g[k].size)
    return [("oracle 2 x 65 x 129", oracle.encode(planes_of("synth", (2, 65, 129), 16))), (f"fixture {names[0]}", g[names[0]].tobytes())]


def truncations(f, count=200):
    return [f[:int(c)] for c in np.linspace(0, len(f) - 1, count).astype(int)]


def corruptions(f, count=500, seed=5):
    """single-byte corruptions of everything that is not block data: boxes, main header, tile-part headers, packet headers"""
    rec = oracle.parse(f)
    is_data = np.zeros(len(f), bool)
    for r in rec[rec[:, F["passes"]] > 0]:
        is_data[r[F["offset"]]:r[F["offset"]] + r[F["length"]]] = True
    where = np.flatnonzero(~is_data)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        pos = int(where[int(rng.integers(len(where)))])
        b = bytearray(f)
        b[pos] ^= int(rng.integers(1, 256)) if k % 3 else (1 << int(rng.integers(8)))
        out.append(bytes(b))
    return out


def check_damaged(L, name, data, room):
    """an error return, or a table that passes the validation the device relies on; never a read behind the buffer (the
    guard page).  Returns the table or None."""
    rc, got = shim_parse(L, data, room=room)
    if rc:
        assert rc in (DEC_BAD, DEC_UNSUPPORTED) and got, (name, rc, got)
        return None
    assert table_is_valid(got, len(data)), name
    return got


def test_truncated_and_corrupted_files_end_in_an_error_or_a_valid_table(shim, golden):
    for name, f in small_files(golden):
        room = GuardedBytes(len(f))
        assert check_damaged(shim, name, f, room) is not None
        errors = tables = 0
        for k, data in enumerate(truncations(f)):
            got = check_damaged(shim, f"{name} cut to {len(data)}", data, room)
            assert got is None, f"{name} cut to {len(data)} of {len(f)} bytes still parses"
            errors += 1
        for k, data in enumerate(corruptions(f)):
            got = check_damaged(shim, f"{name} corruption {k}", data, room)
            errors += got is None
            tables += got is not None
            rc, _ = shim_info(shim, data, room=room)
            assert rc in (0, DEC_BAD, DEC_UNSUPPORTED)
        print(f"{name}: {len(f)} bytes, 200 truncations refused, 500 corruptions: {errors - 200} refused, {tables} parsed to a valid table")


# ------------------------------------------------------------------ host logic

def dec():
    from lbdrn_hip import jp2k_dec
    return jp2k_dec


def test_info_runs_without_a_device_and_refusals_name_the_feature():
    d = dec()
    assert d.available(), f"{DEC_LIB} is not built"
    x = planes_of("synth", (3, 70, 90), 8)
    f = oracle.encode(x)
    assert d.info(f) == (3, 70, 90, 8)
    assert d.info(oracle.encode(planes_of("synth", (1, 1030, 70), 16))) == (1, 1030, 70, 16)
    assert d.lib().lbdrn_jp2kd_workspace(f, len(f)) > 2 * 4 * x.size
    cod = f.index(b"\xff\x52", f.index(b"jp2c"))
    bad = bytearray(f)
    bad[cod + 13] = 0
    with pytest.raises(d.Jp2kDecUnsupported, match="9/7") as e:
        d.info(bytes(bad))
    assert e.value.status == d.E_UNSUPPORTED
    assert d.lib().lbdrn_jp2kd_workspace(bytes(bad), len(bad)) == 0
    with pytest.raises(d.Jp2kDecError) as e:
        d.info(f[:len(f) // 2])
    assert e.value.status == d.E_ARG and not isinstance(e.value, d.Jp2kDecUnsupported)


class _Readers:
    """container._decode_jp2 with both readers replaced: records who was called"""

    def __init__(self, monkeypatch, openjpeg, gpu, gpu_error=None):
        from lbdrn_hip import jp2, jp2k_dec
        self.calls = []
        self.x = np.arange(24, dtype=np.uint16).reshape(2, 3, 4)
        monkeypatch.setattr(jp2, "available", lambda: openjpeg)
        monkeypatch.setattr(jp2k_dec, "available", lambda: gpu)

        def jp2_decode(buf):
            self.calls.append("openjpeg")
            if not openjpeg:
                raise jp2.Jp2Error("liblbdrn_jp2.so not built")
            return self.x

        def gpu_decode(buf, device):
            import torch
            self.calls.append("gpu")
            if gpu_error is not None:
                raise gpu_error
            return torch.from_numpy(self.x.view(np.int16).copy()), 16
        monkeypatch.setattr(jp2, "decode", jp2_decode)
        monkeypatch.setattr(jp2k_dec, "decode", gpu_decode)


SIGNED = b"\x00\x00\x00\x0cjP  \r\n\x87\n" + b"payload"


def test_decode_base_chooses_its_reader_by_LBDRN_BASE_DECODER(monkeypatch):
    from lbdrn_hip import container, jp2, jp2k_dec
    unsupported = jp2k_dec.Jp2kDecUnsupported("lbdrn_jp2kd_info: the irreversible 9/7 transform is not supported", -3)

    def run(value, **kw):
        if value is None:
            monkeypatch.delenv("LBDRN_BASE_DECODER", raising=False)
        else:
            monkeypatch.setenv("LBDRN_BASE_DECODER", value)
        r = _Readers(monkeypatch, **kw)
        try:
            out = container.decode_base(SIGNED, device="cpu")
            assert np.array_equal(out, r.x) and out.dtype == np.uint16
            return r.calls, None
        except Exception as e:      # noqa: BLE001
            return r.calls, e
    # auto (and unset): OpenJPEG where it is built -- today's behaviour --, the GPU decoder where it is not
    for value in (None, "auto", "AUTO"):
        assert run(value, openjpeg=True, gpu=True) == (["openjpeg"], None)
        assert run(value, openjpeg=False, gpu=True) == (["gpu"], None)
        calls, err = run(value, openjpeg=False, gpu=False)
        assert calls == ["openjpeg"] and isinstance(err, jp2.Jp2Error)                       # today's error
        calls, err = run(value, openjpeg=False, gpu=True, gpu_error=unsupported)
        assert calls == ["gpu"] and err is unsupported
    # openjpeg: OpenJPEG only
    assert run("openjpeg", openjpeg=True, gpu=True) == (["openjpeg"], None)
    calls, err = run("openjpeg", openjpeg=False, gpu=True)
    assert calls == ["openjpeg"] and isinstance(err, jp2.Jp2Error)
    # gpu: the GPU decoder; UNSUPPORTED falls back to OpenJPEG where that is built, and raises the library's message where not
    assert run("gpu", openjpeg=True, gpu=True) == (["gpu"], None)
    assert run("gpu", openjpeg=False, gpu=True) == (["gpu"], None)
    assert run("gpu", openjpeg=True, gpu=True, gpu_error=unsupported) == (["gpu", "openjpeg"], None)
    calls, err = run("gpu", openjpeg=False, gpu=True, gpu_error=unsupported)
    assert calls == ["gpu"] and err is unsupported and "9/7" in str(err)
    damaged = jp2k_dec.Jp2kDecError("lbdrn_jp2kd_info: no EOC", -1)
    calls, err = run("gpu", openjpeg=True, gpu=True, gpu_error=damaged)                      # a damaged file is not handed on
    assert calls == ["gpu"] and err is damaged
    calls, err = run("nonsense", openjpeg=True, gpu=True)
    assert calls == [] and isinstance(err, ValueError) and "LBDRN_BASE_DECODER" in str(err)
    # keep_on_device: the GPU path returns the tensor it decoded into, 8-bit files come back as uint8
    monkeypatch.setenv("LBDRN_BASE_DECODER", "gpu")
    r = _Readers(monkeypatch, openjpeg=False, gpu=True)
    t = container.decode_base(SIGNED, device="cpu", keep_on_device=True)
    import torch
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int16 and np.array_equal(t.numpy().view(np.uint16), r.x)
    monkeypatch.setattr(jp2k_dec, "decode", lambda buf, device: (torch.from_numpy(r.x.view(np.int16).copy()), 8))
    out = container.decode_base(SIGNED, device="cpu")
    assert out.dtype == np.uint8 and np.array_equal(out, r.x.astype(np.uint8))
    # a payload of another format never reaches either reader
    with pytest.raises(ValueError):
        container.decode_base(b"XXXXnot a payload")
    assert r.calls == ["gpu"]


def test_library_exports_its_header_only_and_no_kernel_uses_scratch():
    assert os.path.exists(DEC_LIB), f"{DEC_LIB} is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", DEC_LIB], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "lbdrn_jp2k_dec.h")).read()
    declared = set(re.findall(r"\b(lbdrn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"lbdrn_jp2kd_abi_version", "lbdrn_jp2kd_last_error", "lbdrn_jp2kd_info", "lbdrn_jp2kd_workspace", "lbdrn_jp2kd_decode"}
    assert names == declared, (sorted(names - declared), sorted(declared - names))
    assert dec().lib().lbdrn_jp2kd_abi_version() == 1
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump is missing: the kernels' resources cannot be read")
    from kernel_resources import kernel_resources
    rows = kernel_resources(DEC_LIB)
    kernels = {re.sub(r"[<(].*", "", r["demangled"]).split("::")[-1] for r in rows}
    assert kernels == {"k_jp2k_unblocks", "k_jp2k_unlift", "k_jp2k_unshift"}, kernels
    # the criterion tests/test_kernel_disassembly.py holds liblbdrn_hip.so to: no vector register spilled, no scratch memory
    # (scalar registers parked in vector lanes -- k_jp2k_unblocks has some, like k_jp2k_blocks -- touch no memory)
    bad = [(r["demangled"], r["spill_vgpr"], r["scratch"]) for r in rows if r["spill_vgpr"] or r["scratch"]]
    assert not bad, bad
    unblocks = [r for r in rows if "k_jp2k_unblocks" in r["demangled"]]
    assert len(unblocks) == 1 and 19424 <= unblocks[0]["lds"] <= 160 * 1024 // 8, unblocks      # eight blocks per CU (160 KB of LDS)


def test_new_sources_read_no_environment_and_the_hip_header_is_untouched():
    for f in ("jp2k_dec.hip", "jp2k_t1d.inc", "jp2k_t2d.inc"):
        src = open(os.path.join(CSRC, f)).read()
        assert "getenv" not in src and "environ" not in src, f
    hip = open(os.path.join(ROOT, "include", "lbdrn_hip.h")).read()
    assert "jp2kd" not in hip and "jp2kd" not in open(os.path.join(CSRC, "exports.map")).read()
