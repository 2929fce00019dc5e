"""The residual layer restated sequentially in numpy / pure Python, from the format's description (include/lbdrn_resid.h,
DESIGN.md 7): quantiser, fold, the per-row Rice coder, the block layout and the whole LBR1 body, encoder and decoder.
Written from the text, not from csrc/resid.inc: tests/test_resid_host.py and tests/test_gpu_resid.py judge the product
against it.  A plain module: no fixture, no marker."""
import struct

import numpy as np

BLOCK_ROWS, BLOCK_COLS = 64, 256
ESC_Q, RAW_BITS, K_BITS = 24, 17, 4
ESC_BITS = ESC_Q + RAW_BITS
HEADER = 20


class Damaged(ValueError):
    pass


# ---------------------------------------------------------------- quantiser

def quantise(orig, recon, tau):
    """q = sign(e) floor((|e| + tau) / (2 tau + 1)), e = orig - recon; int64 arrays"""
    e = np.asarray(orig, np.int64) - np.asarray(recon, np.int64)
    return np.sign(e) * ((np.abs(e) + tau) // (2 * tau + 1))


def enhance(recon, q, tau, clamp=True):
    v = np.asarray(recon, np.int64) + np.asarray(q, np.int64) * (2 * tau + 1)
    return np.clip(v, 0, 65535) if clamp else v


def fold(q):
    q = np.asarray(q, np.int64)
    return np.where(q >= 0, 2 * q, -2 * q - 1)


def unfold(u):
    u = np.asarray(u, np.int64)
    return np.where(u & 1, -((u + 1) >> 1), u >> 1)


def max_symbol(tau):
    return 2 * ((65535 + tau) // (2 * tau + 1))


# ---------------------------------------------------------------- a row

def symbol_bits(u, k):
    q = u >> k
    return ESC_BITS if q >= ESC_Q else q + 1 + k


def row_costs(us):
    """bits of the row's samples under k = 0..15 (without the 4 bits of k)"""
    us = np.asarray(us, np.int64)
    return [int(np.where(us >> k >= ESC_Q, ESC_BITS, (us >> k) + 1 + k).sum()) for k in range(16)]


def pick_k(us):
    costs = row_costs(us)
    return costs.index(min(costs))        # the lowest k on a tie


def encode_row(us):
    """-> the row as a string of '0' / '1'; '' for a row of zeros"""
    us = [int(u) for u in us]
    if not any(us):
        return ""
    k = pick_k(us)
    out = [format(k, "04b")]
    for u in us:
        q = u >> k
        if q >= ESC_Q:
            out.append("1" * ESC_Q + format(u, "017b"))
        else:
            out.append("1" * q + "0" + (format(u & ((1 << k) - 1), f"0{k}b") if k else ""))
    return "".join(out)


def decode_row(bits, n):
    """the inverse: n samples from exactly these bits; Damaged where they do not hold exactly one row"""
    if bits == "":
        return [0] * n
    if len(bits) <= K_BITS:
        raise Damaged("a row shorter than its parameter")
    k, pos, out = int(bits[:4], 2), 4, []
    for _ in range(n):
        q = 0
        while q < ESC_Q and pos + q < len(bits) and bits[pos + q] == "1":
            q += 1
        if q == ESC_Q:
            raw = bits[pos + ESC_Q:pos + ESC_BITS]
            if len(raw) < RAW_BITS:
                raise Damaged("a row ends inside an escape")
            out.append(int(raw, 2))
            pos += ESC_BITS
        else:
            if pos + q + 1 + k > len(bits):
                raise Damaged("a row ends inside a sample")
            out.append((q << k) | (int(bits[pos + q + 1:pos + q + 1 + k], 2) if k else 0))
            pos += q + 1 + k
    if pos != len(bits):
        raise Damaged("a row does not end where its length says")
    return out


# ---------------------------------------------------------------- blocks and the body

def blocks_of(C, H, W):
    """(c, y0, x0, rows, cols) in the body's order"""
    for c in range(C):
        for y0 in range(0, H, BLOCK_ROWS):
            for x0 in range(0, W, BLOCK_COLS):
                yield c, y0, x0, min(BLOCK_ROWS, H - y0), min(BLOCK_COLS, W - x0)


def encode_block(u):
    """u: [rows][cols] symbols -> bytes"""
    rows = [encode_row(r) for r in u]
    bits = "".join(rows)
    bits += "0" * (-len(bits) % 8)
    return b"".join(struct.pack("<H", len(r)) for r in rows) + (int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b"")


def decode_block(blk, rows, cols, which=None):
    """-> [rows][cols] symbols (rows not in `which` are left zero)"""
    if len(blk) < 2 * rows:
        raise Damaged("a block shorter than its row lengths")
    lens = struct.unpack(f"<{rows}H", blk[:2 * rows])
    if 2 * rows + (sum(lens) + 7) // 8 != len(blk):
        raise Damaged("a block's row lengths do not add up to its bytes")
    data = blk[2 * rows:]
    bits = format(int.from_bytes(data, "big"), f"0{8 * len(data)}b") if data else ""
    out = np.zeros((rows, cols), np.int64)
    pos = 0
    for r in range(rows):
        if which is None or r in which:
            out[r] = decode_row(bits[pos:pos + lens[r]], cols)
        pos += lens[r]
    return out


def header(tau, C, H, W):
    return b"LBR1" + struct.pack("<BBHIII", 1, 0, tau, C, H, W)


def encode_body(orig, recon, tau):
    """orig, recon: [C][H][W] uint16 -> (LBR1 body, recon' as uint16)"""
    orig, recon = np.asarray(orig), np.asarray(recon)
    C, H, W = orig.shape
    q = quantise(orig, recon, tau)
    u = fold(q)
    blocks = [encode_block(u[c, y0:y0 + rows, x0:x0 + cols]) for c, y0, x0, rows, cols in blocks_of(C, H, W)]
    body = header(tau, C, H, W) + b"".join(struct.pack("<I", len(b)) for b in blocks) + b"".join(blocks)
    return body, enhance(recon, q, tau).astype(np.uint16)


def parse_tables(body):
    """-> (tau, C, H, W, [(offset, length) per block]); Damaged for anything inconsistent"""
    if len(body) < HEADER or body[:4] != b"LBR1":
        raise Damaged("not an LBR1 body")
    version, reserved, tau, C, H, W = struct.unpack_from("<BBHIII", body, 4)
    if version != 1 or reserved != 0 or min(C, H, W) < 1 or C > 65535 or max(H, W) > 1 << 20:
        raise Damaged("header")
    geo = list(blocks_of(C, H, W))
    if len(body) < HEADER + 4 * len(geo):
        raise Damaged("table")
    lens = struct.unpack_from(f"<{len(geo)}I", body, HEADER)
    pos, ext = HEADER + 4 * len(geo), []
    for n in lens:
        ext.append((pos, n))
        pos += n
    if pos != len(body):
        raise Damaged("the blocks do not fill the body")
    return tau, C, H, W, ext


def decode_body(body, recon, rect=None):
    """recon: [C][h][w] uint16, the rectangle (x0, y0, w, h) of the tile (None: all of it) -> recon' of that rectangle.
    Only blocks that intersect the rectangle are read."""
    tau, C, H, W, ext = parse_tables(body)
    x0, y0, w, h = rect if rect is not None else (0, 0, W, H)
    out = np.array(recon, dtype=np.int64).reshape(C, h, w)
    for (c, by, bx, rows, cols), (off, n) in zip(blocks_of(C, H, W), ext):
        ya, yb, xa, xb = max(by, y0), min(by + rows, y0 + h), max(bx, x0), min(bx + cols, x0 + w)
        if ya >= yb or xa >= xb:
            continue
        u = decode_block(body[off:off + n], rows, cols, which=set(range(ya - by, yb - by)))
        if int(u.max()) > max_symbol(tau):
            raise Damaged("a symbol beyond the range of tau")
        q = unfold(u)[ya - by:yb - by, xa - bx:xb - bx]
        out[c, ya - y0:yb - y0, xa - x0:xb - x0] = enhance(out[c, ya - y0:yb - y0, xa - x0:xb - x0], q, tau)
    return out.astype(np.uint16)
