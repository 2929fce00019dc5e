"""ctypes binding of liblbdrn_resid.so (include/lbdrn_resid.h): the residual layer "LBR1" -- what separates the original
from the codec's own reconstruction, quantised for a stated maximum error and Rice-coded per row on the GPU
(csrc/resid.hip, csrc/resid.inc).  Built by csrc/build.py beside liblbdrn_hip.so; LBDRN_RESID_LIB names another file."""
import ctypes

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
MAX_TAU = 65535


class ResidError(NativeError):
    pass


_i32, _vp, _sz, _i32p = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_resid.h
    "lbdrn_resid_last_error": (ctypes.c_char_p, []),
    "lbdrn_resid_abi_version": (ctypes.c_int, []),
    "lbdrn_resid_bound": (_sz, [_i32, _i32, _i32]),
    "lbdrn_resid_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_resid_decode_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_resid_encode": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "lbdrn_resid_info": (ctypes.c_int, [ctypes.c_char_p, _sz, _i32p, _i32p, _i32p, _i32p]),
    "lbdrn_resid_decode": (ctypes.c_int, [_vp, _sz, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_resid.so", "LBDRN_RESID_LIB", "lbdrn_resid_", ABI_VERSION, SIGNATURES, ResidError)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


def info(body):
    """(C, H, W, tau) of an LBR1 body; validates its header, block table and row lengths on the host, needs no device."""
    body = bytes(body)
    C, H, W, tau = (ctypes.c_int32() for _ in range(4))
    _check(lib().lbdrn_resid_info(body, len(body), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W), ctypes.byref(tau)), "lbdrn_resid_info")
    return C.value, H.value, W.value, tau.value


def _planes(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dim() != 3 or t.element_size() != 2 or not t.is_contiguous():
        raise ResidError(f"{what}: a contiguous [C,H,W] 16-bit tensor in HBM expected; there is no CPU path in this package")
    return t


def encode(orig, recon, tau):
    """orig, recon: [C,H,W] uint16 planes in HBM (int16 storage, like every plane here) -> the LBR1 body as host bytes.  Runs on
    the current stream of the planes' device; one host sync: the body's length decides how much is copied back."""
    import torch
    orig, recon = _planes(orig, "orig"), _planes(recon, "recon")
    if orig.shape != recon.shape or orig.device != recon.device:
        raise ResidError("orig and recon must have one shape and one device")
    if not 0 <= int(tau) <= MAX_TAU:
        raise ResidError(f"max error {tau} is outside 0..{MAX_TAU}")
    C, H, W = orig.shape
    dev = orig.device
    cap, nws = lib().lbdrn_resid_bound(C, H, W), lib().lbdrn_resid_workspace(C, H, W)
    if not cap or not nws:
        raise ResidError(f"residual layer: geometry {C} x {H} x {W} is out of range")
    with torch.cuda.device(dev):
        body = torch.empty(cap, dtype=torch.uint8, device=dev)
        nbytes = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        _check(lib().lbdrn_resid_encode(orig.data_ptr(), recon.data_ptr(), C, H, W, int(tau), body.data_ptr(), cap, nbytes.data_ptr(),
                                        ws.data_ptr(), nws, torch.cuda.current_stream(dev).cuda_stream), "lbdrn_resid_encode")
        return body[:int(nbytes.item())].cpu().numpy().tobytes()


def apply(body, recon, rect=None):
    """Decode the blocks of `body` (host bytes) that intersect rect = (x0, y0, w, h) of its tile (None: the whole tile) and
    apply them in place to recon, the [C,h,w] planes of that rectangle in HBM.  The body's tables are validated on the host
    first; a damaged body raises.  Returns recon."""
    import torch
    body = bytes(body)
    C, H, W, _ = info(body)
    recon = _planes(recon, "recon")
    x0, y0, w, h = (int(v) for v in rect) if rect is not None else (0, 0, W, H)
    if tuple(recon.shape) != (C, h, w):
        raise ResidError(f"the layer's rectangle is {C} x {h} x {w}, the planes are {tuple(recon.shape)}")
    dev = recon.device
    nws = lib().lbdrn_resid_decode_workspace(C, H, W)
    with torch.cuda.device(dev):
        raw = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        _check(lib().lbdrn_resid_decode(raw.data_ptr(), raw.numel(), C, H, W, x0, y0, w, h, recon.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), nws, torch.cuda.current_stream(dev).cuda_stream), "lbdrn_resid_decode")
        if int(status.item()):
            raise ResidError("the residual layer is inconsistent with its tables (corrupt or truncated body)")
    return recon
