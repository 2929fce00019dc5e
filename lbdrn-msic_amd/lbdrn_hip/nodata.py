"""A scene's nodata value kept exact through lossy coding (encode.py --nodata V): the mask `original == V` of every tile,
coded losslessly beside the tile's payloads, and the decoder's last step, which puts V back where the mask is set and moves
a valid sample that happens to decode to V off it.

No kernel of its own: the mask is a raster of 0 / 1, and the package already has a lossless GPU coder for rasters of small
integers -- lbdrn_plane_encode / lbdrn_plane_decode (LBB2), reached through container.encode_base(codec="LBB2") and
container.decode_base.  Everything else here is elementwise torch work on planes that already lie in HBM.

    tile_mask(orig_d, V) -> (kind, body, count)        the tile's entry of the 'LBNT' chunk (container.pack_nodata_trailer)
    apply(recon_d, kind, body, V, rect=None)           the decoder's mask step, in place
    tau_for(T, V)                                      the residual layer's quantiser bound under --max-error T
    check(orig_d, recon_d, V, T)                       what the encoder asserts before it writes a file

The decode chain of a tile (or of a window's piece), restated in tests/nodata_reference.py:
    r0  the base reconstruction;
    r1  r0 with the residual layer applied, where the file has one and --no-enhancement is absent (else r1 = r0);
    r2  V where the mask is set; where it is clear and r1 == V (the bump), V + 1 -- V - 1 for V = 65535; r1 elsewhere.
So r2 == V exactly where original == V.  Under --max-error T the layer is coded against the original with its nodata samples
replaced by r0 (their error is 0: they cost nothing) with the bound tau_for(T, V): the bump moves a sample by one count, towards
the original when V is 0 or 65535 (the original is not V, so it lies on the bump's side), possibly away from it otherwise.
"""
import struct

import torch

from .container import NODATA_ALL, NODATA_NONE, NODATA_PER_BAND, NODATA_SHARED

MAX_VALUE = 65535


def check_value(V):
    """V as an int; ValueError for anything that is no 16-bit sample value"""
    if isinstance(V, bool) or int(V) != V or not 0 <= int(V) <= MAX_VALUE:
        raise ValueError(f"nodata value {V!r}: a sample value, 0..{MAX_VALUE}")
    return int(V)


def bump_value(V):
    """where a valid sample that decodes to V goes"""
    return V + 1 if V < MAX_VALUE else V - 1


def tau_for(T, V):
    """The bound the residual layer is quantised for so that the chain keeps |original - r2| <= T: T itself at T = 0 (valid
    samples then decode to themselves, never to V) and for V = 0 or 65535 (the bump moves towards the original); T - 1 for an
    interior V, where the bump can add one count."""
    T, V = int(T), check_value(V)
    return T if T == 0 or V in (0, MAX_VALUE) else T - 1


def _stored(v):
    """a 16-bit sample value as the int16 that holds its bits (every plane here: uint16 bits in int16 storage)"""
    return v - 65536 if v >= 32768 else v


def _planes(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dim() != 3 or t.dtype != torch.int16:
        raise ValueError(f"{what}: [C,H,W] uint16 planes in HBM (int16 storage) expected; there is no CPU path in this package")
    return t


def tile_mask(orig_d, V):
    """The mask of one tile's original planes (HBM) -> (kind, body, count of nodata samples): kind 0 / 1 for a tile with no /
    only nodata samples (no body); 2 where every band has the same mask (one plane is coded); 3 otherwise (one per band).
    The body is container.encode_base(the 0/1 planes as uint16, codec="LBB2"): always LBB2, whatever codec the MSB planes get.
    Does not depend on K: the K points of a sweep share it."""
    from . import container
    orig_d, V = _planes(orig_d, "orig"), check_value(V)
    m = orig_d == _stored(V)
    count = int(m.sum().item())
    if count == 0:
        return NODATA_NONE, b"", 0
    if count == m.numel():
        return NODATA_ALL, b"", count
    shared = bool((m == m[:1]).all().item())
    planes = (m[:1] if shared else m).to(torch.int16).contiguous()
    body = container.encode_base(planes, codec="LBB2", device=orig_d.device, as_uint8=False)
    return (NODATA_SHARED if shared else NODATA_PER_BAND), body, count


def decode_mask(kind, body, shape, rect=None, device="cuda:0"):
    """The bool mask of rect = (x0, y0, w, h) of a tile of `shape` = (C, H, W) (None: the whole tile), broadcastable to
    [C,h,w]; None for kind 0, True for kind 1.  The payload has no partial mode: decoded whole, cropped on the device like
    the MSB planes of a window."""
    from . import container
    C, H, W = shape
    if kind == NODATA_NONE:
        return None
    if kind == NODATA_ALL:
        return True
    if kind not in (NODATA_SHARED, NODATA_PER_BAND):
        raise ValueError(f"nodata mask of kind {kind}")
    if bytes(body[:4]) != container.BASE_LBB2_MAGIC:
        raise ValueError("nodata mask: the body is no LBB2 payload")
    planes = container.decode_base(bytes(body), device=device, keep_on_device=True)
    want = (1 if kind == NODATA_SHARED else C, H, W)
    if tuple(planes.shape) != want:
        raise ValueError(f"nodata mask of kind {kind}: the body holds {tuple(planes.shape)} planes, the tile needs {want}")
    if rect is not None:
        x0, y0, w, h = (int(v) for v in rect)
        if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError(f"nodata mask: rectangle x0={x0} y0={y0} w={w} h={h} is not inside the {W} x {H} tile")
        planes = planes[:, y0:y0 + h, x0:x0 + w]
    return planes != 0


def apply(recon_d, kind, body, V, rect=None):
    """The decoder's mask step, in place on recon_d: the [C][h][w] planes (HBM) of rect = (x0, y0, w, h) of the tile, None =
    the whole tile.  Returns recon_d."""
    recon_d, V = _planes(recon_d, "recon"), check_value(V)
    C, h, w = recon_d.shape
    if rect is not None and (int(rect[2]), int(rect[3])) != (w, h):
        raise ValueError(f"the mask's rectangle is {rect[3]} x {rect[2]}, the planes are {h} x {w}")
    if kind == NODATA_ALL:
        return recon_d.fill_(_stored(V))
    m = None
    if kind != NODATA_NONE:
        if len(body) < 15:
            raise ValueError(f"nodata mask: a body of {len(body)} bytes")
        H, W = struct.unpack_from(">II", bytes(body[7:15]), 0)      # LBB2's frame: magic, code u8, C u16, H u32, W u32
        if rect is None and (H, W) != (h, w):
            raise ValueError(f"nodata mask: the body is {H} x {W}, the planes are {h} x {w}")
        m = decode_mask(kind, body, (C, H, W), rect, recon_d.device)
    bumped = recon_d == _stored(V)
    if m is not None:
        bumped &= ~m
    recon_d.masked_fill_(bumped, _stored(bump_value(V)))
    if m is not None:
        recon_d.masked_fill_(m.expand_as(recon_d), _stored(V))
    return recon_d


def merge_original(orig_d, recon_d, V):
    """orig': the original with its nodata samples replaced by the reconstruction's -- what the residual layer is coded
    against under --nodata, so that those samples have error 0 and rows of nothing else cost no bits"""
    return torch.where(orig_d == _stored(check_value(V)), recon_d, orig_d).contiguous()


def check(orig_d, recon_d, V, T=None):
    """What the encoder asserts on the chain's result before a file is written: recon == V exactly where orig == V, and with a
    bound T, max |orig - recon| <= T.  -> that maximum.  Raises ValueError."""
    V = check_value(V)
    wrong = int(((orig_d == _stored(V)) != (recon_d == _stored(V))).sum().item())
    if wrong:
        raise ValueError(f"nodata: {wrong} samples decode to {V} without being nodata, or are nodata and do not; no bitstream is written")
    err = int((orig_d.to(torch.int32) & 0xFFFF).sub_(recon_d.to(torch.int32) & 0xFFFF).abs_().max().item())
    if T is not None and err > T:
        raise ValueError(f"nodata: max error {err} after the mask step, {T} was asked for; no bitstream is written")
    return err
