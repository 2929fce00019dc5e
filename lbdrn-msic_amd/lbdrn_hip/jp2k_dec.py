"""ctypes binding of liblbdrn_jp2k_dec.so (include/lbdrn_jp2k_dec.h): the GPU decoder of the lossless JPEG 2000 MSB payload
(csrc/jp2k_dec.hip).  Reads what `jp2-gpu` writes and what OpenJPEG and Pillow write with reversible settings,
without OpenJPEG, and leaves the planes in HBM.  Files with a precinct partition (COD's Scod bit 0) and with the
reversible component transform (mct = 1 on three components or more) are read as well.  Built by csrc/build.py beside liblbdrn_hip.so; LBDRN_JP2K_DEC_LIB
names another file."""
import ctypes

import numpy as np

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
MAX_SAMPLES = 1 << 33


class Jp2kDecError(NativeError):
    pass


class Jp2kDecUnsupported(Jp2kDecError):
    """the file is a JPEG 2000 stream this decoder does not take (LBDRN_E_UNSUPPORTED); the message names the feature"""


_i32, _vp, _sz, _buf, _i32p = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_jp2k_dec.h
    "lbdrn_jp2kd_last_error": (ctypes.c_char_p, []),
    "lbdrn_jp2kd_abi_version": (ctypes.c_int, []),
    "lbdrn_jp2kd_info": (ctypes.c_int, [_buf, _sz, _i32p, _i32p, _i32p, _i32p]),
    "lbdrn_jp2kd_workspace": (_sz, [_buf, _sz]),
    "lbdrn_jp2kd_decode": (ctypes.c_int, [_buf, _sz, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_jp2k_dec.so", "LBDRN_JP2K_DEC_LIB", "lbdrn_jp2kd_", ABI_VERSION, SIGNATURES, Jp2kDecError)
lib, available, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.path


def _check(rc, what):
    if rc != 0:
        raise (Jp2kDecUnsupported if rc == E_UNSUPPORTED else Jp2kDecError)(f"{what}: {_NATIVE.last_error()}", rc)


def info(buf):
    """(C, H, W, bits) of a .jp2 file or raw codestream; validates the whole file on the host, needs no device.  Raises
    Jp2kDecUnsupported for a stream outside the accepted subset, Jp2kDecError for a damaged one."""
    buf = bytes(buf)
    C, H, W, bits = (ctypes.c_int32() for _ in range(4))
    _check(lib().lbdrn_jp2kd_info(buf, len(buf), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W), ctypes.byref(bits)), "lbdrn_jp2kd_info")
    return C.value, H.value, W.value, bits.value


def decode(buf, device):
    """.jp2 file or raw codestream (host bytes) -> ([C,H,W] uint16 planes in HBM: int16 storage with the same bits, the
    storage ops.plane_decode returns; the file's precision in bits).  Runs on the current stream of `device`, which the
    call synchronises."""
    import torch
    buf = bytes(buf)
    C, H, W, bits = info(buf)
    if C * H * W > MAX_SAMPLES:
        raise Jp2kDecError(f"implausible JPEG 2000 geometry {C} x {H} x {W}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise Jp2kDecError("liblbdrn_jp2k_dec works on device (HBM) tensors only; there is no CPU path in this package")
    nws = lib().lbdrn_jp2kd_workspace(buf, len(buf))
    with torch.cuda.device(dev):
        planes = torch.empty((C, H, W), dtype=torch.int16, device=dev)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        _check(lib().lbdrn_jp2kd_decode(buf, len(buf), ctypes.c_void_p(planes.data_ptr()), C, H, W, ctypes.c_void_p(ws.data_ptr()), nws,
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lbdrn_jp2kd_decode")
    return planes, bits


def decode_numpy(buf, device):
    """-> [C,H,W] numpy uint8 (precision <= 8) or uint16, as jp2.decode returns"""
    planes, bits = decode(buf, device)
    x = planes.cpu().numpy().view(np.uint16)
    return x.astype(np.uint8) if bits <= 8 else x
