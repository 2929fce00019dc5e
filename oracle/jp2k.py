"""ctypes wrapper of oracle/jp2k_oracle.c (the JPEG 2000 oracle: encode, decode, parse, and the stages on their own) and
of oracle/jp2k_host_shim.cpp (the product's host-compilable tier-1 / tier-2 text).  TEST INFRASTRUCTURE."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import build as _build  # noqa: E402

FIELDS = ("tile", "comp", "res", "band", "gx", "gy", "numbps", "passes", "offset", "length", "mb", "x", "y", "w", "h", "orient")
F = {n: k for k, n in enumerate(FIELDS)}
COUNTERS = ("rl_exit0", "rl_exit1", "rl_exit2", "rl_exit3", "rl_zero", "partial_stripe", "narrow_block", "passes_16bit", "lblock_inc",
            "header_stuff", "tree_not_pow2", "empty_band_beside_full", "empty_packet", "pass_row0", "pass_row1", "pass_row2",
            "pass_row3", "pass_row4", "excluded_in_full_packet")

_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
_lib = None
_shim = None


class Jp2kOracleError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_build.build())
        L.jo_last_error.restype = ctypes.c_char_p
        L.jo_counters.argtypes = [_vp, _i]
        L.jo_counters.restype = None
        L.jo_dwt53.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _i]
        L.jo_t1_encode.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]
        L.jo_t1_decode.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _i]
        L.jo_blocks.argtypes = [_i, _i, _i, _i, _vp, _i64]
        L.jo_blocks.restype = _i64
        L.jo_layout.argtypes = [_i, _i, _i, _i, _vp]
        L.jo_packet_header_write.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _sz]
        L.jo_packet_header_write.restype = _i64
        L.jo_packet_header_parse.argtypes = [_i, _vp, _vp, _vp, _vp, _sz, _vp]
        L.jo_packet_header_parse.restype = _i64
        L.jo_coefficients.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp]
        L.jo_encode.argtypes = [_vp, _i, _i, _i, _i, _vp, _sz]
        L.jo_encode.restype = _i64
        L.jo_info.argtypes = [_vp, _sz, _vp]
        L.jo_parse.argtypes = [_vp, _sz, _vp, _i64]
        L.jo_parse.restype = _i64
        L.jo_decode.argtypes = [_vp, _sz, _vp]
        _lib = L
    return _lib


def _fail(what):
    raise Jp2kOracleError(f"{what}: {lib().jo_last_error().decode(errors='replace')}")


def _p(a):
    return a.ctypes.data_as(_vp)


def counters(reset=False):
    """{name: how often the oracle took that path since the last reset}"""
    out = np.zeros(24, np.uint64)
    lib().jo_counters(_p(out), int(reset))
    return {n: int(out[k]) for k, n in enumerate(COUNTERS)}


def _planes(x):
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    if x.dtype not in (np.uint8, np.uint16):
        raise ValueError("planes must be uint8 or uint16")
    return np.ascontiguousarray(x.astype(np.uint16)), (8 if x.dtype == np.uint8 else 16)


# ------------------------------------------------------------------ stages

def dwt53(a, levels, x0=0, y0=0, inverse=False):
    """[h, w] int32 -> its 5/3 transform in the Mallat layout (or back), the first sample at (x0, y0) of the grid"""
    a = np.array(a, dtype=np.int32, order="C")
    h, w = a.shape
    if lib().jo_dwt53(_p(a), w, h, w, x0, y0, levels, int(inverse)):
        _fail("jo_dwt53")
    return a


def t1_encode(coef, orient, cap=None):
    """[h, w] int32 coefficients of a code block -> (bytes, passes, numbps)"""
    coef = np.ascontiguousarray(coef, dtype=np.int32)
    h, w = coef.shape
    room = w * h * 18 + 4096 if cap is None else cap
    out = np.zeros(max(room, 1), np.uint8)
    passes, numbps = ctypes.c_int32(), ctypes.c_int32()
    n = lib().jo_t1_encode(_p(coef), w, w, h, orient, _p(out), room, ctypes.byref(passes), ctypes.byref(numbps))
    if n < 0 or (cap is None and n > room):
        _fail("jo_t1_encode")
    return out[:min(n, room)].tobytes(), passes.value, numbps.value


def t1_decode(data, w, h, orient, numbps, passes):
    data = np.frombuffer(bytes(data) + b"\0", np.uint8)
    out = np.zeros((h, w), np.int32)
    if lib().jo_t1_decode(_p(data), len(data) - 1, w, h, orient, numbps, passes, _p(out), w):
        _fail("jo_t1_decode")
    return out


def blocks(C, H, W, bits=16):
    """the block table of the encoder's geometry, in packet order: int64 [n, 16], columns FIELDS"""
    n = lib().jo_blocks(C, H, W, bits, None, 0)
    if n < 0:
        _fail("jo_blocks")
    rec = np.zeros((n, len(FIELDS)), np.int64)
    lib().jo_blocks(C, H, W, bits, _p(rec), n)
    return rec


def layout(C, H, W, bits=16):
    """(tiles across, tiles down, tile width, tile height, resolutions)"""
    out = np.zeros(5, np.int32)
    if lib().jo_layout(C, H, W, bits, _p(out)):
        _fail("jo_layout")
    return tuple(int(v) for v in out)


def coefficients(x, tile, comp):
    """the transformed coefficients of one tile-component: int32 [tile height, tile width], Mallat layout"""
    x, bits = _planes(x)
    C, H, W = x.shape
    ntx, nty, tw, th, _ = layout(C, H, W, bits)
    w = min(tw, W - (tile % ntx) * tw)
    h = min(th, H - (tile // ntx) * th)
    out = np.zeros((h, w), np.int32)
    if lib().jo_coefficients(_p(x), C, H, W, bits, tile, comp, _p(out)):
        _fail("jo_coefficients")
    return out


def _bands(gw, gh, mb):
    return tuple(np.ascontiguousarray(v, dtype=np.int32) for v in (gw, gh, mb))


def packet_header_write(gw, gh, mb, rec):
    """bands of gw[b] x gh[b] blocks announcing mb[b] planes; rec int32 [blocks, 3]: passes, numbps, bytes -> header bytes"""
    gw, gh, mb = _bands(gw, gh, mb)
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(64 + 32 * len(rec), np.uint8)
    n = lib().jo_packet_header_write(len(gw), _p(gw), _p(gh), _p(mb), _p(rec), _p(out), out.size)
    if n < 0 or n > out.size:
        _fail("jo_packet_header_write")
    return out[:n].tobytes()


def packet_header_parse(gw, gh, mb, data):
    """-> (rec int32 [blocks, 3], bytes of the header)"""
    gw, gh, mb = _bands(gw, gh, mb)
    nblk = int((gw.astype(np.int64) * gh).sum())
    rec = np.zeros((max(nblk, 1), 3), np.int32)
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    n = lib().jo_packet_header_parse(len(gw), _p(gw), _p(gh), _p(mb), _p(buf), len(buf) - 1, _p(rec))
    if n < 0:
        _fail("jo_packet_header_parse")
    return rec[:nblk], int(n)


# ------------------------------------------------------------------ whole files

def encode(x):
    """[C, H, W] uint8 / uint16 -> the .jp2 file as bytes"""
    x, bits = _planes(x)
    C, H, W = x.shape
    cap = x.size * 3 + 64 * len(blocks(C, H, W, bits)) + 4096
    out = np.zeros(cap, np.uint8)
    n = lib().jo_encode(_p(x), C, H, W, bits, _p(out), cap)
    if n < 0 or n > cap:
        _fail("jo_encode")
    return out[:n].tobytes()


def info(buf):
    """{C, H, W, bits, tiles, blocks, resolutions, tw, th} of a .jp2 file or raw codestream"""
    a = np.frombuffer(bytes(buf), np.uint8)
    out = np.zeros(9, np.int64)
    if lib().jo_info(_p(a), a.size, _p(out)):
        _fail("jo_info")
    return dict(zip(("C", "H", "W", "bits", "tiles", "blocks", "resolutions", "tw", "th"), (int(v) for v in out)))


def parse(buf):
    """one record per code block, in packet order: int64 [n, 16], columns FIELDS (offset into buf; -1 and passes 0
    for a block the file does not include)"""
    a = np.frombuffer(bytes(buf), np.uint8)
    n = info(buf)["blocks"]
    rec = np.zeros((max(n, 1), len(FIELDS)), np.int64)
    if lib().jo_parse(_p(a), a.size, _p(rec), n) != n:
        _fail("jo_parse")
    return rec[:n]


def decode(buf):
    """-> [C, H, W] uint8 (precision <= 8) or uint16"""
    a = np.frombuffer(bytes(buf), np.uint8)
    i = info(buf)
    out = np.zeros((i["C"], i["H"], i["W"]), np.uint16)
    if lib().jo_decode(_p(a), a.size, _p(out)):
        _fail("jo_decode")
    return out.astype(np.uint8) if i["bits"] <= 8 else out


def tile_parts(buf):
    """the bytes from the first SOT to the end of the file (what is left when the main header, COM included, is gone)"""
    buf = bytes(buf)
    at = buf.index(b"jp2c") + 4 if buf[:4] != b"\xff\x4f\xff\x51" else 0
    assert buf[at:at + 2] == b"\xff\x4f"
    at += 2
    while buf[at:at + 2] != b"\xff\x90":
        at += 2 + int.from_bytes(buf[at + 2:at + 4], "big")
    return buf[at:]


def first_difference(a, b, x=None):
    """where two files of the same planes part: '' when equal, else a sentence that names the first differing code block
    (tile, component, resolution, band, gx, gy), which of numbps / passes / length / bytes differ, and -- given the planes
    x and taking b as the oracle's file -- whether the oracle's tier-1 decoding of a's block gives the oracle's own
    coefficients (then a's coder is at fault; otherwise its transform or staging)."""
    a, b = bytes(a), bytes(b)
    if a == b:
        return ""
    try:
        ra, rb = parse(a), parse(b)
    except Jp2kOracleError as e:
        return f"files differ ({len(a)} / {len(b)} bytes) and one does not parse: {e}"
    if ra.shape != rb.shape or not np.array_equal(ra[:, [F[k] for k in ("tile", "comp", "res", "band", "gx", "gy", "x", "y", "w", "h", "orient", "mb")]],
                                                  rb[:, [F[k] for k in ("tile", "comp", "res", "band", "gx", "gy", "x", "y", "w", "h", "orient", "mb")]]):
        return f"files differ in their geometry or headers: {info(a)} / {info(b)}"
    for p, q in zip(ra, rb):
        da = a[p[F["offset"]]:p[F["offset"]] + p[F["length"]]] if p[F["passes"]] else b""
        db = b[q[F["offset"]]:q[F["offset"]] + q[F["length"]]] if q[F["passes"]] else b""
        what = [k for k in ("numbps", "passes", "length") if p[F[k]] != q[F[k]]] + (["bytes"] if da != db else [])
        if not what:
            continue
        where = ", ".join(f"{k} {int(p[F[k]])}" for k in ("tile", "comp", "res", "band", "gx", "gy"))
        msg = (f"first differing code block: {where} ({int(p[F['w']])} x {int(p[F['h']])}, orientation {int(p[F['orient']])}): "
               f"{' and '.join(what)} differ (numbps {int(p[F['numbps']])} / {int(q[F['numbps']])}, passes {int(p[F['passes']])} / "
               f"{int(q[F['passes']])}, length {int(p[F['length']])} / {int(q[F['length']])})")
        if x is not None:
            co = coefficients(x, int(p[F["tile"]]), int(p[F["comp"]]))
            want = co[p[F["y"]]:p[F["y"]] + p[F["h"]], p[F["x"]]:p[F["x"]] + p[F["w"]]]
            try:
                got = t1_decode(da, int(p[F["w"]]), int(p[F["h"]]), int(p[F["orient"]]), int(p[F["numbps"]]), int(p[F["passes"]]))
                same = np.array_equal(got, want)
            except Jp2kOracleError:
                same = False
            msg += ("; the oracle's tier-1 decoder reads the oracle's coefficients from the first file's block: its block CODER is at fault"
                    if same else "; the oracle's tier-1 decoder reads other coefficients from the first file's block than the oracle's: "
                                 "its TRANSFORM or STAGING is at fault (or its coder, beyond decodability)")
        return msg
    return f"every code block agrees, the files differ outside them (headers, packet headers or order): {len(a)} / {len(b)} bytes"


# ------------------------------------------------------------------ the product's host text (oracle/jp2k_host_shim.cpp)

def shim():
    """the host shim's library, or None where no C++ compiler built it"""
    global _shim
    if _shim is None:
        path = _build.build_jp2k_host_shim()
        if path is None:
            return None
        L = ctypes.CDLL(path)
        L.jp2k_shim_code_block.argtypes = [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]
        L.jp2k_shim_blocks.argtypes = [_i, _i, _i, _i, _vp, _i64]
        L.jp2k_shim_blocks.restype = _i64
        L.jp2k_shim_packet_header.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _sz]
        L.jp2k_shim_packet_header.restype = _i64
        L.jp2k_shim_assemble.argtypes = [_i, _i, _i, _i, _vp, _vp, ctypes.c_uint64, _vp, _sz]
        L.jp2k_shim_assemble.restype = _i64
        _shim = L
    return _shim


def shim_code_block(coef, orient, cap=None, canary=64):
    """the product's block coder -> (the first min(bytes, cap) bytes, reported bytes, passes, numbps); asserts that the
    `canary` bytes behind the buffer are untouched"""
    coef = np.ascontiguousarray(coef, dtype=np.int32)
    h, w = coef.shape
    room = w * h * 18 + 4096 if cap is None else cap
    out = np.full(room + canary, 0xA5, np.uint8)
    passes, numbps = ctypes.c_int32(), ctypes.c_int32()
    n = shim().jp2k_shim_code_block(_p(coef), w, w, h, orient, _p(out), room, ctypes.byref(passes), ctypes.byref(numbps))
    assert n >= 0
    assert (out[room:] == 0xA5).all(), "the block coder wrote beyond its capacity"
    return out[:min(n, room)].tobytes(), n, passes.value, numbps.value


def shim_blocks(C, H, W, bits=16):
    """the product's block table: int64 [n, 8]: slab, x, y, w, h, orient, mb, cap"""
    n = shim().jp2k_shim_blocks(C, H, W, bits, None, 0)
    assert n >= 0, (C, H, W, bits, n)
    rec = np.zeros((max(n, 1), 8), np.int64)
    assert shim().jp2k_shim_blocks(C, H, W, bits, _p(rec), n) == n
    return rec[:n]


def shim_packet_header(gw, gh, mb, rec):
    gw, gh, mb = _bands(gw, gh, mb)
    rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(64 + 32 * len(rec), np.uint8)
    n = shim().jp2k_shim_packet_header(len(gw), _p(gw), _p(gh), _p(mb), _p(rec), _p(out), out.size)
    assert 0 <= n <= out.size
    return out[:n].tobytes()


def shim_assemble(C, H, W, bits, res, data):
    """res uint32 [blocks, 4]: bytes, passes, numbps, 0; data: the blocks' bytes back to back -> the file"""
    res = np.ascontiguousarray(res, dtype=np.uint32)
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    need = shim().jp2k_shim_assemble(C, H, W, bits, _p(res), None, 0, None, 0)
    out = np.zeros(need, np.uint8)
    n = shim().jp2k_shim_assemble(C, H, W, bits, _p(res), _p(buf), len(buf) - 1, _p(out), need)
    assert n == need
    return out.tobytes()
