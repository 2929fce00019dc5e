"""encode.py --nodata restated in numpy, from its description (lbdrn_hip/nodata.py's docstring): the mask, the
decoder's mask step, the bound the residual layer is quantised for, the whole decode chain with tests/resid_reference.py's
quantiser, and the 'LBNT' chunk's bytes.  Written from the text, not from the product's code: tests/test_nodata_host.py and
tests/test_gpu_nodata.py judge the product against it.  A plain module: no fixture, no marker."""
import struct

import numpy as np

import resid_reference as R

TOP = 65535


def mask(orig, V):
    return np.asarray(orig) == V


def bump_value(V):
    return V + 1 if V < TOP else V - 1


def tau_for(T, V):
    """T at T = 0 and for V at either end of the range (the bump moves towards the original), else T - 1"""
    return T if T == 0 or V in (0, TOP) else T - 1


def mask_step(r1, m, V):
    """r2: V where the mask is set; where it is clear and r1 == V, the bump; r1 elsewhere"""
    r1 = np.asarray(r1, np.int64)
    return np.where(m, V, np.where(r1 == V, bump_value(V), r1))


def merged_original(orig, r0, V):
    """orig': the original with its nodata samples replaced by the base reconstruction's"""
    return np.where(mask(orig, V), np.asarray(r0, np.int64), np.asarray(orig, np.int64))


def chain(orig, r0, V, T=None, masked=True, tau=None):
    """-> (r2, r1, tau) of the decode chain for an original and its base reconstruction; T None: a file without a residual
    layer (r1 = r0, tau None).  masked=False: decode.py --no-mask (r2 = r1).  tau: quantise for this bound instead of the
    rule's (to show what the rule is for)."""
    orig, r0 = np.asarray(orig, np.int64), np.asarray(r0, np.int64)
    if T is None:
        r1 = r0
    else:
        tau = tau_for(T, V) if tau is None else tau
        r1 = R.enhance(r0, R.quantise(merged_original(orig, r0, V), r0, tau), tau)
    return (mask_step(r1, mask(orig, V), V) if masked else r1), r1, tau


def tile_kind(orig, V):
    """0: no nodata sample, 1: nothing else, 2: every band has the same mask, 3: otherwise -> (kind, the 0/1 planes coded)"""
    m = mask(orig, V)
    if not m.any():
        return 0, None
    if m.all():
        return 1, None
    if (m == m[:1]).all():
        return 2, m[:1].astype(np.uint16)
    return 3, m.astype(np.uint16)


def pack_chunk(V, entries, version=1, reserved=0):
    """'LBNT' | version u8 | reserved u8 | V u16 | per tile: kind u8, size u32 | the bodies; big-endian.  entries: [(kind, body)]"""
    out = b"LBNT" + struct.pack(">BBH", version, reserved, V)
    for kind, body in entries:
        out += struct.pack(">BI", kind, len(body))
    return out + b"".join(body for _, body in entries)
