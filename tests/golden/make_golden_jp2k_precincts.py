"""Writes tests/golden/jp2k_precincts.npz: small reversible .jp2 files written by Pillow (OpenJPEG) with what the other
JPEG 2000 fixture lacks -- an explicit precinct partition (COD's Scod bit 0 and one size byte per resolution) and the
reversible component transform (COD's mct byte) -- and the samples Pillow reads back from them, so that the GPU decoder's
packet walk and its inverse RCT (csrc/jp2k_t2d.inc, csrc/jp2k_dec.hip) are judged against an independent writer and
reader where neither is present.

    python tests/golden/make_golden_jp2k_precincts.py

Pillow only.  The content is seeded: smooth planes plus a little noise, so the files stay small.  Every case asserts
that Pillow reads back what went in, that COD announces a partition where the case is about precincts (Pillow drops the
partition silently when the precinct is not at least twice the code block) and that mct is 1 where it is about the RCT.
tests/test_jp2k_dec_precincts_host.py imports CASES, planes_of_case and write_case to regenerate the files live."""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name, (C, H, W), dtype, top value, Pillow's settings, has a precinct partition, mct
CASES = (
    ("u8_1x40x50_cb4_prec8", (1, 40, 50), np.uint8, 255,
     dict(num_resolutions=3, codeblock_size=(4, 4), precinct_size=(8, 8)), True, 0),
    ("u16_1x150x200_res6_prec32", (1, 150, 200), np.uint16, 2047,
     dict(num_resolutions=6, precinct_size=(32, 32)), True, 0),
    ("u8_3x150x200_rct_res4_prec32x256", (3, 150, 200), np.uint8, 255,
     dict(mct=1, num_resolutions=4, precinct_size=(32, 256)), True, 1),
    ("u8_3x150x200_prec64_cb32", (3, 150, 200), np.uint8, 255,
     dict(mct=0, precinct_size=(64, 64), codeblock_size=(32, 32)), True, 0),
    ("u8_3x150x200_rct", (3, 150, 200), np.uint8, 255,
     dict(mct=1), False, 1),
    ("u8_3x150x200_tiled96x80_prec64_cb32_rct", (3, 150, 200), np.uint8, 255,
     dict(tile_size=(96, 80), precinct_size=(64, 64), codeblock_size=(32, 32), mct=1), True, 1),
)


def planes_of_case(k):
    """[C, H, W]: a smooth surface per component (components differ, so the RCT has chroma to carry) plus noise of a few
    levels, inside [0, top]"""
    name, (C, H, W), dtype, top, kw, prec, mct = CASES[k]
    rng = np.random.default_rng(20261017 + k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((C, H, W), dtype)
    for c in range(C):
        s = 0.5 + 0.3 * np.sin(x / (17.0 + 5 * c) + c) * np.cos(y / (23.0 - 3 * c)) + 0.15 * (x + (c + 1) * y) / (W + (c + 1) * H)
        v = s * top * 0.8 + rng.integers(-3, 4, (H, W))
        out[c] = np.clip(np.rint(v), 0, top).astype(dtype)
    return out


def cod_of(f):
    """(Scod, mct, the precinct bytes) of the main header's COD"""
    at = f.index(b"jp2c") + 4
    assert f[at:at + 2] == b"\xff\x4f"
    at += 2
    while f[at:at + 2] != b"\xff\x90":
        n = int.from_bytes(f[at + 2:at + 4], "big")
        if f[at:at + 2] == b"\xff\x52":
            return f[at + 4], f[at + 8], bytes(f[at + 14:at + 2 + n])
        at += 2 + n
    raise AssertionError("no COD")


def write_case(k):
    """-> (the file Pillow writes for case k, the samples Pillow reads back from it as [C, H, W])"""
    from PIL import Image
    name, (C, H, W), dtype, top, kw, prec, mct = CASES[k]
    x = planes_of_case(k)
    buf = io.BytesIO()
    Image.fromarray(x[0] if C == 1 else np.ascontiguousarray(x.transpose(1, 2, 0))).save(buf, "JPEG2000", irreversible=False, **kw)
    f = buf.getvalue()
    im = Image.open(io.BytesIO(f))
    im.load()
    back = np.asarray(im).astype(dtype)
    back = np.ascontiguousarray(back[None] if C == 1 else back.transpose(2, 0, 1))
    assert np.array_equal(back, x), f"{name}: Pillow does not read back what it was given"
    scod, m, sizes = cod_of(f)
    assert bool(scod & 1) == prec, f"{name}: Scod {scod:#x}, a precinct partition was {'expected' if prec else 'not expected'}"
    assert len(sizes) == (kw.get("num_resolutions", 6) if prec else 0), (name, sizes.hex())
    assert m == mct, f"{name}: mct {m}, expected {mct}"
    return f, back


def main():
    import PIL
    from PIL import features
    out = {"pillow_version": np.array(PIL.__version__), "openjpeg_version": np.array(str(features.version_codec("jpg_2000")))}
    for k, case in enumerate(CASES):
        f, back = write_case(k)
        out["file_" + case[0]] = np.frombuffer(f, np.uint8)
        out["planes_" + case[0]] = back
        print(f"{case[0]}: {len(f)} bytes, COD precinct bytes {cod_of(f)[2].hex(' ') or '-'}, mct {cod_of(f)[1]}")
    path = os.path.join(HERE, "jp2k_precincts.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "OpenJPEG", features.version_codec("jpg_2000"))


if __name__ == "__main__":
    main()
