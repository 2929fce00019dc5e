/* liblbdrn_plane3.so -- "LBB3", the lossless payload of the MSB planes with inter-band prediction, coded and decoded on
 * the GPU from and to the planes where they lie in HBM (csrc/plane3.hip, csrc/plane3.inc), plain C ABI.
 *
 * LBB3 is LBB2 (csrc/plane_codec.hip) with two changes: the unit of work holds all bands of its pixels, so that a band can
 * be predicted from the band before it, and a band of a pass picks one of eight modes instead of four.  The entropy stage
 * -- adaptive Golomb-Rice per lane with zero-group flags, the 32-bit words of a unit interleaved in the order the decoding
 * wave asks for them -- is LBB2's, and one text with it: both are built from csrc/plane_lane.inc (predictors, fold, lane
 * coder) and csrc/plane_wave.hpp (the wave's walk).  For one band and S >= H a unit is an LBB2 strip, and the body behind
 * the header is LBB2's body byte for byte.  container.py frames the body as b"LBB3" + pack(">BHII", code, C, H, W) + body.
 *
 * ---------------------------------------------------------------------------------------------------------- the format
 *
 * A body is a sequence of 32-bit little-endian words; its bytes are a function of the planes (and S) alone.
 *
 *     header, 5 words    'L' 'B' 'P' '3' | C | H | W | S
 *                        1 <= C <= 16 bands, 1 <= H, W <= 2^20, S a multiple of 64 in 64 .. 2^20 (the writer: S = 256).
 *     table              one word per unit: the number of words of that unit.
 *     units              back to back, in table order.
 *
 * Units.  The raster is cut into units of 64 columns x S rows x all C bands, narrower at the right edge and shorter at the
 * bottom edge: TX = ceil(W / 64) units in a row of units, NU = ceil(H / S) rows of units, unit (uy, ux) at table index
 * uy * TX + ux.  A unit of tw columns and uh rows is decoded by one wave of 64 lanes, alone: nothing outside the unit is
 * used to predict it and every coder state starts anew.
 *
 * A unit is walked in passes of 64 rows (the last one shorter: rows = min(64, uh - 64 p)); lane i owns row 64 p + i of
 * the unit.  Within a pass the bands follow one another, band 0 first; within a band the wave walks the anti-diagonals:
 * at step d = 0 .. rows + tw - 2, lane i < rows decodes column j = d - i of its row if 0 <= j < tw.  When band c of a pass
 * is decoded, band c - 1 of that pass is complete.
 *
 *     unit               C head words, band c's at index c:  k0 | z0 << 12  (k0 <= 15, z0 <= 2, every other bit zero);
 *                        then per pass: ceil(C / 10) mode words -- band c's mode in bits 3 (c % 10) .. 3 (c % 10) + 2 of
 *                        word c / 10, every unused bit zero -- followed, band by band, by the words the lanes take.
 *
 * The words the lanes take.  Every lane reads one bit stream of its own, MSB first, continuous over the bands and passes of
 * the unit.  Before it decodes a symbol, a lane that holds fewer than 32 unread bits takes the unit's next word and appends
 * it to what it holds; the lanes that take at the same step take consecutive words in lane order.  (A symbol is at most 32
 * bits, so a lane never needs more than one word a step.)  A lane's stream is padded with zero bits; a word a lane takes
 * beyond its last coded bit is zero.  The unit ends with the last word taken: its word count is exact.
 *
 * Prediction.  x is the sample, a its left neighbour, b the one above, d the one above-left, all of the same band, as
 * integers 0 .. 65535.  The four spatial predictors P_m(a, b, d):
 *     m = 0  MED     d >= max(a, b) ? min(a, b) : d <= min(a, b) ? max(a, b) : a + b - d
 *     m = 1  mean    (a + b) >> 1
 *     m = 2  plane   a + b - d
 *     m = 3  mix     ((3 (a + b) - 2 d + 2^20) >> 2) - 2^18          (the floor of (3 (a + b) - 2 d) / 4)
 * Borders, by the position in the UNIT: the unit's first row is predicted from the left only (P = a, and P = 0 for its first
 * sample), the first column of every other row from above only (P = b).  These rules replace P_m where they apply.
 * Mode m = 0 .. 3 (plain) predicts x_c by P_m(a_c, b_c, d_c).  Mode 4 + m (differential, bands c >= 1 only) predicts it by
 *     P_m(a_c, b_c, d_c) + (x_{c-1} - P_m(a_{c-1}, b_{c-1}, d_{c-1}))
 * at the same pixel of the band before, with the same border rules in both bands: the band before's residual under the same
 * spatial predictor is carried over.  Band 0's mode is 0 .. 3.
 * The residual is e = (x - prediction) modulo 2^16, read as a signed 16-bit number, folded to v = e >= 0 ? 2 e : -2 e - 1.
 * The decoder forms x = (prediction + e) modulo 2^16.
 *
 * The lane coder.  Every lane keeps one state (A, N) per band; it starts a unit as N = 4 and A = 0 (z0 = 2), 1 (z0 = 1) or
 * 6 << k0 (z0 = 0), with the k0, z0 of the band's head word.  A row (one band of one pass, for one lane) starts outside any
 * group.  Per sample, in column order:
 *     outside a group    g = 16 if 16 A < N, 4 if 2 A < N, else 1.  If g > 1: g = min(g, tw - j), and one flag bit follows --
 *                        0: the next g samples of the row are all v = 0 and take no further bits; 1: they are coded.
 *                        The group lasts g samples.
 *     a coded sample     k = the smallest value in 0 .. 15 with (N << (k + 1)) >= A (15 if there is none); q = v >> k;
 *                        q < 15: q one-bits, a zero bit, the k low bits of v;  q >= 15: 15 one-bits and v in 16 bits.
 *     after every sample A += v, N += 1, and at N = 32: A = (A + 1) >> 1, N = 16.
 *
 * What the writer chooses.  Per (unit, pass, band) the mode with the smallest sum of v over the pass, the lower index on a
 * tie.  k0, z0 of a band from that smallest sum `best` of the unit's first pass and count = rows * tw: k0 the smallest value
 * in 0 .. 15 with (count << (k0 + 1)) >= best (15 if none), z0 = 2 if 16 best < count, 1 if 2 best < count, else 0.  A
 * reader takes any head word and mode the ranges above allow.
 *
 * ---------------------------------------------------------------------------------------------------------- the calls
 *
 * Conventions are those of lbdrn_resid.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_plane3_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); the device
 * calls enqueue on it and do not synchronise.  The workspace's contents do not matter on entry, nothing beyond the stated
 * sizes is written, and a short workspace or capacity is LBDRN_E_WORKSPACE before any launch.
 *
 *   lbdrn_plane3_bound             the most bytes a body of this geometry can take under the writer's S (0: out of range)
 *   lbdrn_plane3_encode_workspace  device scratch bytes lbdrn_plane3_encode needs (the lanes' private streams, the symbol
 *                                  lengths and the units before compaction)
 *   lbdrn_plane3_decode_workspace  what lbdrn_plane3_decode needs for a body of this geometry and any S: 8 bytes per unit
 *                                  of the finest cut (S = 64) and a word
 *   lbdrn_plane3_encode            planes: DEVICE [C][H][W] uint16.  body (DEVICE, 4-byte aligned, capacity >=
 *                                  lbdrn_plane3_bound) receives the body, *body_bytes (DEVICE u64) its length.
 *   lbdrn_plane3_info              HOST only, needs no device: validates the header and the unit table of a body in host
 *                                  memory against its length -- magic, ranges, S, a table that fits, counts within what a
 *                                  unit of that size can take, counts that add up to exactly the body -- and returns the
 *                                  geometry and S.
 *   lbdrn_plane3_decode            body: DEVICE, 4-byte aligned, n bytes, for the C x H x W and S the caller states (from
 *                                  lbdrn_plane3_info, before the body went to the device).  planes: DEVICE [C][H][W] uint16,
 *                                  every sample written.  *status (DEVICE int32) is set to 0, then
 *                                  to non-zero where the body is damaged: a header that is not this geometry's, a table
 *                                  that overruns the body or does not add up to it, a head or mode word out of range, a unit whose lanes ask for
 *                                  more or fewer words than its count.  A damaged body gives status != 0 or planes of
 *                                  unspecified values; it never makes the decoder read outside body[0, n) or write outside
 *                                  planes, status and the workspace, and every iteration of every loop produces a sample
 *                                  or ends the unit.
 */
#ifndef LBDRN_PLANE3_H
#define LBDRN_PLANE3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_PLANE3_ABI_VERSION 1

const char *lbdrn_plane3_last_error(void);
int lbdrn_plane3_abi_version(void);
size_t lbdrn_plane3_bound(int32_t C, int32_t H, int32_t W);
size_t lbdrn_plane3_encode_workspace(int32_t C, int32_t H, int32_t W);
size_t lbdrn_plane3_decode_workspace(int32_t C, int32_t H, int32_t W);
int lbdrn_plane3_encode(const uint16_t *planes, int32_t C, int32_t H, int32_t W, void *body, size_t capacity, uint64_t *body_bytes,
                        void *workspace, size_t workspace_bytes, void *stream);
int lbdrn_plane3_info(const void *body, size_t n, int32_t *C, int32_t *H, int32_t *W, int32_t *S);
int lbdrn_plane3_decode(const void *body, size_t n, int32_t C, int32_t H, int32_t W, int32_t S, uint16_t *planes, int32_t *status,
                        void *workspace, size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
