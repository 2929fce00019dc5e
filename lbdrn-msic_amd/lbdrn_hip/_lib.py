"""ctypes binding of liblbdrn_hip.so (C ABI: include/lbdrn_hip.h)."""
import ctypes

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library  # noqa: F401  (enum lbdrn_status)

ABI_VERSION = 2           # LBDRN_ABI_VERSION of include/lbdrn_hip.h this binding was written against
PATH_AUTO, PATH_GENERIC, PATH_MFMA = 0, 1, 2
EVAL_BACKGROUND = 0x200   # hint OR'ed into `path` of lbdrn_eval_sse
EVAL_FAST = 0x400         # the per-epoch ranking pass in the tolerance arithmetic (lbdrn_hip.h)
EVAL_X16 = 0x1000         # with EVAL_FAST, opt-in: layer 0's colour features on the f16 matrix pipe, operands exact (lbdrn_hip.h)
EVAL_VALID = 0x4000        # lbdrn_geom.reserved holds a nodata value: samples equal to it add no term to the sum (lbdrn_hip.h)
EVAL_DECODED = 0x8000      # the closed-loop sum: a term is (img - out)^2, out the sample lbdrn_decode_fused writes; exact (lbdrn_hip.h)
APPLY_DECODE = 0x2000   # path word of lbdrn_apply_instance only: the request lbdrn_decode_fused makes (lbdrn_hip.h)
TRAIN_ALONE = 0x800      # hint OR'ed into `path` of lbdrn_train_epoch: nothing else in flight on the device (lbdrn_hip.h)


class LbdrnError(RuntimeError):
    """A failed library call; `code` is the lbdrn_status it returned (None for host-side failures)."""
    code = None


class Geom(ctypes.Structure):
    """struct lbdrn_geom"""
    _fields_ = [("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("K", ctypes.c_int32), ("D", ctypes.c_int32), ("msb_max", ctypes.c_int32),
                ("use_colors", ctypes.c_int32), ("relative", ctypes.c_int32),
                ("P", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rowtab", ctypes.c_void_p), ("coltab", ctypes.c_void_p)]


class Net(ctypes.Structure):
    """struct lbdrn_net"""
    _fields_ = [("F", ctypes.c_int32), ("bc", ctypes.c_int32), ("C", ctypes.c_int32),
                ("nl", ctypes.c_int32), ("act", ctypes.c_int32)]


# name -> (restype, argtypes); must list every symbol include/lbdrn_hip.h declares
_vp, _i32, _i64, _sz, _dbl = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t,
                              ctypes.c_double)
_GP, _NP = ctypes.POINTER(Geom), ctypes.POINTER(Net)
SIGNATURES = {
    "lbdrn_last_error": (ctypes.c_char_p, []),
    "lbdrn_abi_version": (ctypes.c_int, []),
    "lbdrn_device_check": (ctypes.c_int, []),
    "lbdrn_param_count": (_i64, [_NP]),
    "lbdrn_feature_dim": (_i32, [_GP]),
    "lbdrn_split_bits": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lbdrn_labels": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "lbdrn_features": (ctypes.c_int, [_GP, _vp, _vp, _i64, _vp, _vp]),
    "lbdrn_forward_workspace": (_sz, [_NP, _i64]),
    "lbdrn_forward": (ctypes.c_int, [_NP, _vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "lbdrn_tape_bytes": (_sz, [_NP, _i64]),
    "lbdrn_forward_tape": (ctypes.c_int, [_NP, _vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "lbdrn_backward_workspace": (_sz, [_NP, _i64]),
    "lbdrn_backward": (ctypes.c_int, [_NP, _vp, _vp, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "lbdrn_apply_workspace": (_sz, [_GP, _NP]),
    "lbdrn_decode_fused": (ctypes.c_int, [_GP, _NP, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "lbdrn_eval_sse": (ctypes.c_int, [_GP, _NP, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "lbdrn_apply_instance": (ctypes.c_int, [_GP, _NP, _i32, ctypes.POINTER(_i32)]),
    "lbdrn_train_workspace": (_sz, [_GP, _NP, _i32]),
    "lbdrn_train_prepare": (ctypes.c_int, [_GP, _NP, _vp, _vp, _i32, _vp, _sz, _i32, _vp]),
    "lbdrn_train_epoch": (ctypes.c_int, [_GP, _NP, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64,
                                         _dbl, _vp, _vp, _sz, _i32, _vp]),
    "lbdrn_train_group_max": (ctypes.c_int, []),
    "lbdrn_train_step_features": (_i32, [_GP, _NP]),
    "lbdrn_train_group_size": (_i32, [_GP, _NP]),
    "lbdrn_train_epoch_group": (ctypes.c_int, [_i32, _vp, _NP, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _dbl, _vp,
                                               _vp, _sz, _i32, _vp]),
    "lbdrn_train_profile_mode": (ctypes.c_int, [_i32]),
    "lbdrn_randperm_workspace": (_sz, [_i64, _i32]),
    "lbdrn_randperm": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), _i32, _i64, _vp, _vp, _sz, _vp]),
    "lbdrn_mt19937_jump_poly": (_i64, [_i32, _vp]),
    "lbdrn_plane_bound": (_sz, [_i32, _i32, _i32]),
    "lbdrn_plane_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_plane_encode": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "lbdrn_plane_decode": (ctypes.c_int, [_vp, _sz, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "lbdrn_jp2k_block_count": (_i64, [_i32, _i32, _i32]),
    "lbdrn_jp2k_bound": (_sz, [_i32, _i32, _i32]),
    "lbdrn_jp2k_workspace": (_sz, [_i32, _i32, _i32]),
    "lbdrn_jp2k_encode": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _sz, ctypes.POINTER(ctypes.c_size_t), _vp, _sz, _vp]),
    "lbdrn_weights_bound": (_sz, [_i64]),
    "lbdrn_weights_encode": (ctypes.c_int, [_vp, _i64, _i32, _vp, _sz, ctypes.POINTER(ctypes.c_size_t)]),
    "lbdrn_weights_info": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "lbdrn_weights_decode": (ctypes.c_int, [_vp, _sz, _vp, _i64]),
    "lbdrn_train_step": (ctypes.c_int, [_NP, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _dbl, _i32, _vp,
                                        _vp, _vp, _sz, _vp]),
}

# LBDRN_HIP_LIB selects another build of the same ABI (e.g. the diagnostic liblbdrn_hip_stamps.so)
_NATIVE = Library("liblbdrn_hip.so", "LBDRN_HIP_LIB", "lbdrn_", ABI_VERSION, SIGNATURES, LbdrnError,
                  missing="{path} is missing: build it with `python lbdrn-msic_amd/csrc/build.py` "
                          "(hipcc, gfx950).  This package has no CPU fallback.",
                  mismatch="liblbdrn_hip ABI {got} != {want}")


def lib_path():
    return _NATIVE.path


def lib():
    """Load liblbdrn_hip.so.  torch must be imported first so that the HIP runtime torch ships
    (same SONAME, libamdhip64.so.7) is the one both sides use."""
    if _NATIVE.loaded is None:
        import torch  # noqa: F401  (loads libamdhip64 first)
        _NATIVE.lib()
    return _NATIVE.loaded


def check(rc):
    if rc != 0:
        err = LbdrnError(f"liblbdrn_hip error {rc}: {_NATIVE.last_error()}")
        err.code = rc
        raise err
