"""ctypes binding of liblbdrn_plane3.so (include/lbdrn_plane3.h): "LBB3", the lossless MSB payload with inter-band
prediction, coded and decoded on the GPU (csrc/plane3.hip, csrc/plane3.inc).  Built by csrc/build.py beside
liblbdrn_hip.so; LBDRN_PLANE3_LIB names another file."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.environ.get("LBDRN_PLANE3_LIB") or os.path.join(os.path.dirname(_HERE), "liblbdrn_plane3.so")
ABI_VERSION = 1
E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4      # lbdrn_status of include/lbdrn_hip.h
MAX_BANDS = 16

_lib = None


class Plane3Error(RuntimeError):
    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise Plane3Error(f"{_PATH} not built (python lbdrn-msic_amd/csrc/build.py)")
        L = ctypes.CDLL(_PATH)
        i32, vp, sz = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.lbdrn_plane3_last_error.restype = ctypes.c_char_p
        L.lbdrn_plane3_abi_version.restype = ctypes.c_int
        for name in ("lbdrn_plane3_bound", "lbdrn_plane3_encode_workspace", "lbdrn_plane3_decode_workspace"):
            getattr(L, name).argtypes = [i32, i32, i32]
            getattr(L, name).restype = sz
        L.lbdrn_plane3_encode.argtypes = [vp, i32, i32, i32, vp, sz, vp, vp, sz, vp]
        L.lbdrn_plane3_info.argtypes = [ctypes.c_char_p, sz, i32p, i32p, i32p, i32p]
        L.lbdrn_plane3_decode.argtypes = [vp, sz, i32, i32, i32, i32, vp, vp, vp, sz, vp]
        if L.lbdrn_plane3_abi_version() != ABI_VERSION:
            raise Plane3Error(f"{_PATH}: ABI version {L.lbdrn_plane3_abi_version()}, this binding is for {ABI_VERSION}")
        _lib = L
    return _lib


def available():
    try:
        lib()
        return True
    except (Plane3Error, OSError):
        return False


def _check(rc, what):
    if rc != 0:
        raise Plane3Error(f"{what}: {(lib().lbdrn_plane3_last_error() or b'').decode(errors='replace')}", rc)


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
