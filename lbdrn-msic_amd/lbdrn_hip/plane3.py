"""ctypes binding of liblbdrn_plane3.so (include/lbdrn_plane3.h): "LBB3", the lossless MSB payload with inter-band
prediction, coded and decoded on the GPU (csrc/plane3.hip, csrc/plane3.inc).  Built by csrc/build.py beside
liblbdrn_hip.so; LBDRN_PLANE3_LIB names another file."""
import ctypes

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
MAX_BANDS = 16


class Plane3Error(NativeError):
    pass


_i32, _vp, _sz, _i32p = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_plane3.h
    "lbdrn_plane3_last_error": (ctypes.c_char_p, []),
    "lbdrn_plane3_abi_version": (ctypes.c_int, []),
    "lbdrn_plane3_bound": (_sz, [_i32, _i32, _i32]),
    "lbdrn_plane3_encode_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_plane3_decode_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_plane3_encode": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "lbdrn_plane3_info": (ctypes.c_int, [ctypes.c_char_p, _sz, _i32p, _i32p, _i32p, _i32p]),
    "lbdrn_plane3_decode": (ctypes.c_int, [_vp, _sz, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_plane3.so", "LBDRN_PLANE3_LIB", "lbdrn_plane3_", ABI_VERSION, SIGNATURES, Plane3Error)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


def info(body):
    """(C, H, W, S) of an LBB3 body; validates its header and unit table against its length on the host, needs no device."""
    body = bytes(body)
    C, H, W, S = (ctypes.c_int32() for _ in range(4))
    _check(lib().lbdrn_plane3_info(body, len(body), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W), ctypes.byref(S)), "lbdrn_plane3_info")
    return C.value, H.value, W.value, S.value


def _planes(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dim() != 3 or t.element_size() != 2:
        raise Plane3Error(f"{what}: a [C,H,W] 16-bit tensor in HBM expected; there is no CPU path in this package")
    return t.contiguous()


def encode(planes):
    """[C,H,W] uint16 planes in HBM (int16 storage, like every plane here) -> the LBB3 body as host bytes.  Runs on the current
    stream of the planes' device; one host sync: the body's length decides how much is copied back."""
    import torch
    planes = _planes(planes, "planes")
    C, H, W = planes.shape
    if C > MAX_BANDS:
        raise ValueError(f"LBB3 codes at most {MAX_BANDS} bands, the planes have {C}")
    dev = planes.device
    cap, nws = lib().lbdrn_plane3_bound(C, H, W), lib().lbdrn_plane3_encode_workspace(C, H, W)
    if not cap or not nws:
        raise Plane3Error(f"LBB3: geometry {C} x {H} x {W} is out of range")
    with torch.cuda.device(dev):
        body = torch.empty(cap, dtype=torch.uint8, device=dev)
        nbytes = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        _check(lib().lbdrn_plane3_encode(planes.data_ptr(), C, H, W, body.data_ptr(), cap, nbytes.data_ptr(), ws.data_ptr(), nws,
                                         torch.cuda.current_stream(dev).cuda_stream), "lbdrn_plane3_encode")
        return body[:int(nbytes.item())].cpu().numpy().tobytes()


def decode(body, C, H, W, device):
    """LBB3 body (host bytes) for the geometry its frame names -> [C,H,W] uint16 planes in HBM (int16 storage).  The header
    and the unit table are validated on the host first; a damaged body raises."""
    import torch
    body = bytes(body)
    bC, bH, bW, S = info(body)
    if (bC, bH, bW) != (C, H, W):
        raise Plane3Error(f"the LBB3 body is {bC} x {bH} x {bW}, its frame says {C} x {H} x {W}")
    dev = torch.device(device)
    nws = lib().lbdrn_plane3_decode_workspace(C, H, W)
    with torch.cuda.device(dev):
        raw = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
        planes = torch.empty((C, H, W), dtype=torch.int16, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        _check(lib().lbdrn_plane3_decode(raw.data_ptr(), raw.numel(), C, H, W, S, planes.data_ptr(), status.data_ptr(), ws.data_ptr(), nws,
                                         torch.cuda.current_stream(dev).cuda_stream), "lbdrn_plane3_decode")
        if int(status.item()):
            raise Plane3Error("LBB3 payload is inconsistent with its tables (corrupt or truncated stream)")
    return planes
