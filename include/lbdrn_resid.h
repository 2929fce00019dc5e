/* liblbdrn_resid.so -- the residual (enhancement) layer of the codec, coded and decoded on the GPU (csrc/resid.hip,
 * csrc/resid.inc), plain C ABI.
 *
 * The codec's reconstruction is canonical arithmetic: every decoder of this package computes the same uint16 raster
 * from the same MSB planes and weight payload.  The encoder therefore knows `recon` bit for bit and codes what separates
 * it from the original, in a closed loop, for a maximum error tau >= 0 the user states (tau = 0: lossless).
 *
 * Semantics, per sample (orig, recon uint16; e = orig - recon):
 *     q      = sign(e) * floor((|e| + tau) / (2 tau + 1))
 *     recon' = clamp(recon + q (2 tau + 1), 0, 65535)            |orig - recon'| <= tau, always
 *     u      = q >= 0 ? 2 q : -2 q - 1                            the coded symbol, 0 <= u <= 2 floor((65535 + tau) / (2 tau + 1))
 * No predictor: the network is the predictor.
 *
 * Body format "LBR1" (all integers little-endian; the bytes are a function of (orig, recon, tau) alone):
 *     header, 20 bytes   'L' 'B' 'R' '1' | version u8 = 1 | reserved u8 = 0 | tau u16 | C u32 | H u32 | W u32
 *                        (the reserved byte keeps the table on a 4-byte offset)
 *     block table        one u32 byte length per block.  A plane is cut into blocks of 64 rows x 256 columns, smaller at
 *                        the right and bottom edges; blocks in raster order per plane, planes in order.
 *     blocks             back to back, in table order.  A block is
 *                          one u16 bit length per row present,
 *                          the rows' bit streams concatenated MSB-first (a row starts at the bit the one before ended),
 *                          zero bits up to the next byte.
 *                        Its byte length is exactly 2 rows + ceil(sum of the row lengths / 8).
 *     a row of zeros     has length 0 and no bits.
 *     any other row      4 bits k (the Rice parameter: the value in 0..15 that gives the fewest bits, the lowest on a tie),
 *                        then per sample: (u >> k) one-bits, a zero bit, the k low bits of u -- or, where u >> k >= 24,
 *                        24 one-bits and u in 17 bits.  A row is at most 4 + 256 * 41 = 10500 bits: the bound a reader
 *                        accepts and lbdrn_resid_bound counts.  (What lbdrn_resid_encode writes is at most
 *                        4 + 256 * 19 = 4868 bits a row: it takes the cheapest k, and under k = 15 no sample needs more
 *                        than 3 + 1 + 15 bits.)
 * Blocks are independent: a rectangle is decoded from the blocks it intersects and the table.
 *
 * Conventions are those of lbdrn_jp2k_dec.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_resid_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); the device
 * calls enqueue on it and do not synchronise.  The workspace's contents do not matter on entry, nothing beyond the stated
 * sizes is written, and a short workspace or capacity is LBDRN_E_WORKSPACE before any launch.
 * Alignment (LBDRN_E_ARG before any launch otherwise): the workspace 256 bytes -- its regions are 32- and 64-bit words at
 * multiples of 256 from the base --, orig, recon and recon_inout 2, status 4, body_bytes 8.  The body needs none: it is
 * read and written bytewise.
 *
 *   lbdrn_resid_bound      the most bytes a body of this geometry can take (0: geometry out of range -- C <= 65535,
 *                          H, W <= 2^20)
 *   lbdrn_resid_workspace  device scratch bytes lbdrn_resid_encode needs for this geometry (the lanes' private streams,
 *                          sized by the 4868 bits a coded row can reach: 38 KB per block).  lbdrn_resid_decode_workspace: what lbdrn_resid_decode needs (the table and
 *                          its scan: 12 bytes per block), so that a window decode does not allocate for an encode.
 *   lbdrn_resid_encode     orig, recon: DEVICE [C][H][W] uint16.  One pass forms e, q, u and codes them; body (DEVICE,
 *                          capacity >= lbdrn_resid_bound) receives the body, *body_bytes (DEVICE u64) its length.
 *   lbdrn_resid_info       HOST only, needs no device: validates the header, the block table and every block's row
 *                          lengths of a body in host memory and returns its geometry and tau.
 *   lbdrn_resid_decode     body: DEVICE, n bytes.  Decodes only the blocks that intersect the rectangle (x0, y0, w, h) of
 *                          the C x H x W tile and applies recon' in place to recon_inout, DEVICE [C][h][w] uint16: the
 *                          rectangle's samples (the whole tile is (0, 0, W, H)).  *status (DEVICE int32) is set to 0, then
 *                          to non-zero where the body is damaged: a header that is not this geometry's, a table that
 *                          overruns the body, row lengths that do not add up, a row that does not end where its length
 *                          says, a symbol beyond the range of tau.  A damaged body gives status != 0 or a raster of
 *                          unspecified values; every read of body is bounded by the validated extent of its block, and
 *                          nothing outside recon_inout, status and the workspace is written.
 */
#ifndef LBDRN_RESID_H
#define LBDRN_RESID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_RESID_ABI_VERSION 1

const char *lbdrn_resid_last_error(void);
int lbdrn_resid_abi_version(void);
size_t lbdrn_resid_bound(int32_t C, int32_t H, int32_t W);
size_t lbdrn_resid_workspace(int32_t C, int32_t H, int32_t W);
size_t lbdrn_resid_decode_workspace(int32_t C, int32_t H, int32_t W);
int lbdrn_resid_encode(const uint16_t *orig, const uint16_t *recon, int32_t C, int32_t H, int32_t W, int32_t tau, void *body,
                       size_t capacity, uint64_t *body_bytes, void *workspace, size_t workspace_bytes, void *stream);
int lbdrn_resid_info(const void *body, size_t n, int32_t *C, int32_t *H, int32_t *W, int32_t *tau);
int lbdrn_resid_decode(const void *body, size_t n, int32_t C, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
                       uint16_t *recon_inout, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
