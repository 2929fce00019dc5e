"""Precinct partitions and the reversible component transform in the GPU JPEG 2000 decoder (lbdrn_jp2kd_decode,
csrc/jp2k_dec.hip) on the device: every file of tests/golden/jp2k_precincts.npz (written by Pillow / OpenJPEG) decodes to
what Pillow reads from it, through the C ABI and through container.decode_base, from poisoned guarded buffers; the RCT
form of k_jp2k_unshift on more than three components, which Pillow cannot write (the oracle's files of transformed
planes with COD's mct byte set); damaged files.  Every comparison is exact.  A mismatch names the first differing
component, tile and sample, and whether the product's own block table reconstructs the planes on the CPU (then the
device kernels are at fault, k_jp2k_unshift's RCT form among them) or not (then the table is)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import jp2k as oracle  # noqa: E402
from guarded import Arena, fill_id  # noqa: E402
from test_jp2k_dec_host import GuardedBytes, load_shim  # noqa: E402
from test_jp2k_dec_precincts_host import (check_damaged, corruptions, describe_difference, fixture_cases, forward_rct, main_header,  # noqa: E402
                                          reconstruct, smallest_two, truncations)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def gpu_reader(monkeypatch):
    monkeypatch.setenv("LBDRN_BASE_DECODER", "gpu")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


def dec():
    from lbdrn_hip import jp2k_dec
    return jp2k_dec


def guarded_decode(f, dev, fill=0xA5):
    """lbdrn_jp2kd_decode into guarded buffers pre-filled with `fill` -> [C, H, W] uint8 / uint16; asserts the guards"""
    import torch
    d = dec()
    L = d.lib()
    C, H, W, bits = d.info(f)
    nws = L.lbdrn_jp2kd_workspace(f, len(f))
    assert nws > 0, (L.lbdrn_jp2kd_last_error() or b"").decode()
    arena = Arena(dev)
    ws = arena.buf(nws, fill, name="workspace")
    out = arena.buf(C * H * W * 2, fill, name="planes")
    rc = L.lbdrn_jp2kd_decode(f, len(f), out.ptr, C, H, W, ws.ptr, nws, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert rc == 0, (L.lbdrn_jp2kd_last_error() or b"").decode()
    arena.check()
    got = out.numpy(np.uint16).reshape(C, H, W)
    return got.astype(np.uint8) if bits <= 8 else got


def explain(shim, f, got, want):
    h = main_header(f)
    host = reconstruct(shim, f)
    side = ("the product's block table reconstructs the expected planes on the CPU: the DEVICE kernels are at fault"
            + (" (k_jp2k_unshift<true>, the inverse RCT, among them)" if h["mct"] else "")) if np.array_equal(host, want) else \
        "the product's block table does not reconstruct the expected planes on the CPU either: the TABLE (jp2k_t2d.inc) is at fault"
    return f"{describe_difference(h, got, want)}; {side}"


def assert_equal_planes(shim, label, f, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        raise AssertionError(f"jp2k-dec {label}: {explain(shim, f, got, want)}")


def test_every_fixture_file_decodes_to_what_pillow_reads(dev, golden, shim):
    for name, f, want in fixture_cases(golden):
        assert_equal_planes(shim, name, f, guarded_decode(f, dev), want)


def test_every_fixture_file_decodes_through_decode_base(dev, golden, shim, monkeypatch):
    import torch
    from lbdrn_hip import container, jp2

    def no_openjpeg(buf):
        raise AssertionError("decode_base handed the file to OpenJPEG: the GPU decoder refused it")
    monkeypatch.setattr(jp2, "decode", no_openjpeg)
    for name, f, want in fixture_cases(golden):
        assert_equal_planes(shim, f"decode_base {name}", f, container.decode_base(f, device=dev), want)
    name, f, want = fixture_cases(golden)[2]
    t = container.decode_base(f, device=dev, keep_on_device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint16), want)


@pytest.mark.parametrize("fill", (0xA5, 0x00), ids=fill_id)
def test_same_bits_from_poisoned_guarded_buffers(fill, dev, golden, shim):
    for name, f, want in fixture_cases(golden):
        assert_equal_planes(shim, f"{name} {fill_id(fill)}", f, guarded_decode(f, dev, fill), want)


def rct_case(C, bits):
    """planes [C, 90, 130] of `bits` significant bits whose first three components lie closer together than half the
    file's range (|c0 - c1|, |c2 - c1| < 2^(precision - 1): the transformed chroma then fits the file's unsigned
    samples), and the planes a writer with mct = 1 would code for them: G.2.1 on the level-shifted components 0 - 2,
    shifted back; the others as they are"""
    rng = np.random.default_rng(1000 * C + bits)
    dtype, precision = (np.uint8, 8) if bits <= 8 else (np.uint16, 16)
    top, H, W = (1 << bits) - 1, 90, 130
    x = rng.integers(0, top + 1, (C, H, W)).astype(np.int64)
    if precision == 8:          # components 0 and 2 within +-100 of component 1
        yy, xx = np.mgrid[0:H, 0:W]
        x[1] = np.clip(128 + 90 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.integers(-20, 21, (H, W)), 0, top)
        x[0] = np.clip(x[1] + rng.integers(-100, 101, (H, W)), 0, top)
        x[2] = np.clip(x[1] + rng.integers(-100, 101, (H, W)), 0, top)
    half = 1 << (precision - 1)
    assert np.abs(x[0] - x[1]).max() < half and np.abs(x[2] - x[1]).max() < half
    y = x.copy()
    y[:3] = forward_rct(x[:3] - half) + half
    assert y.min() >= 0 and y.max() < (1 << precision), "the transformed planes do not fit the file's samples"
    assert (y[1] < half).any() and (y[1] > half).any() and ((y[1] + y[2] - 2 * half) % 4 != 0).any()      # both signs, a floor that matters
    return x.astype(dtype), y.astype(dtype)


@pytest.mark.parametrize("C,bits", ((4, 8), (8, 11)), ids=("C4_8bits", "C8_11bits"))
def test_rct_on_more_than_three_components(C, bits, dev, shim):
    x, y = rct_case(C, bits)
    plain = oracle.encode(y)
    h = main_header(plain)
    assert h["mct"] == 0 and h["C"] == C
    f = bytearray(plain)
    f[h["cod"] + 8] = 1
    f = bytes(f)
    assert np.array_equal(guarded_decode(plain, dev), y)             # the unpatched file: the plain kernel, every component as coded
    got = guarded_decode(f, dev)
    assert_equal_planes(shim, f"RCT on {C} components of {bits} bits", f, got, x)
    assert np.array_equal(got[3:], y[3:]) and np.array_equal(got[3:], guarded_decode(plain, dev, 0x00)[3:])


def test_a_mismatch_names_component_tile_and_sample(dev, golden, shim):
    name, f, want = fixture_cases(golden)[5]                         # tiles of 96 x 80, mct = 1
    got = guarded_decode(f, dev)
    assert np.array_equal(got, want)
    other = want.copy()
    other[1, 85, 100] ^= 1                                           # tile 4: second row, second column of three
    msg = explain(shim, f, got, other)
    assert "first in component 1, tile 4 at sample (y 85, x 100)" in msg and "inverse RCT" in msg and "TABLE" in msg, msg
    assert "DEVICE" in explain(shim, f, other, want)


def test_damaged_precinct_files_give_an_error_or_a_raster_with_the_guards_intact(dev, golden, shim):
    """50 truncations and 100 header corruptions of the smallest precinct file -- each first through the CPU build of the
    same parser (behind a guard page), then once through the device: an error, or a raster of some values; never a
    write outside the buffers.  The host refuses what it cannot validate before any launch."""
    import torch
    d = dec()
    L = d.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    name, f, _ = smallest_two(golden)[0]
    room = GuardedBytes(len(f))
    ran = refused = 0
    for k, data in enumerate(truncations(f, 50) + corruptions(shim, f, 100, seed=12)):
        table = check_damaged(shim, f"{name} damaged {k}", data, room)
        try:
            c2, h2, w2, _ = d.info(data)
        except d.Jp2kDecError:
            assert table is None, f"{name} damaged {k}: the library refuses what its host text parses"
            refused += 1
            continue
        assert table is not None
        need = L.lbdrn_jp2kd_workspace(data, len(data))
        if c2 * h2 * w2 > 1 << 24 or need > 1 << 28:      # (a corrupted size field: not worth the memory)
            continue
        arena = Arena(dev)
        ws = arena.buf(need, 0xA5, name="workspace")
        out = arena.buf(c2 * h2 * w2 * 2, 0xA5, name="planes")
        rc = L.lbdrn_jp2kd_decode(data, len(data), out.ptr, c2, h2, w2, ws.ptr, need, stream)
        torch.cuda.synchronize(dev)
        assert rc in (0, d.E_ARG, d.E_UNSUPPORTED), (name, k, rc)
        arena.check()
        ran += 1
    print(f"damaged precinct files: {refused} refused on the host, {ran} decoded on the device")
    assert ran > 0 and refused > 0
