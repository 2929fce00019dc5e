/* liblbdrn_quality.so -- two rasters that lie in HBM compared on the GPU (csrc/quality.hip, csrc/quality.inc), plain C ABI:
 * exact per-band error statistics with the error histogram, SSIM per band, and the spectral angle (SAM) per pixel.
 *
 * a and b are DEVICE rasters of C planes, H rows and W samples of unsigned 8 or 16 bits, unit sample stride, row and plane
 * strides in samples (a_row, b_row >= W): a window of a larger scene is compared where it lies.  e = a - b as integers.
 *
 * The result (DEVICE, lbdrn_quality_result_bytes(C) bytes, 8-byte aligned; every field 8 bytes, little-endian):
 *   C band records of 264 fields (2112 bytes), band c at byte 2112 c:
 *     u64 n           H * W
 *     u64 sse         sum of e^2               (below 2^63: H * W <= 2^31)
 *     u64 sae         sum of |e|
 *     i64 sum_err     sum of e
 *     u64 max_abs     max of |e|
 *     u64 hist[257]   hist[k] = #{|e| = k} for k < 256, hist[256] = #{|e| >= 256}
 *     u64 ssim_n      windows counted: (H - 10)(W - 10), or 0 where H < 11, W < 11 or SSIM was not asked for
 *     f64 ssim_sum    sum of the windows' SSIM
 *   one pixel record of 4 fields behind them, at byte 2112 C:
 *     u64 sam_n          pixels with an angle
 *     u64 sam_undefined  pixels where a (or b) is zero in every band and the other is not
 *     f64 sam_sum        sum of the angles, radians
 *     f64 sam_max        the largest angle
 * The integer fields are exact.  Fields of a part that `what` does not select are zero.
 *
 * SSIM (what & LBDRN_QUALITY_SSIM), per band, all in float64: separable Gaussian window of 11 taps, sigma 1.5, weights
 * normalised to sum 1; moments mu_a, mu_b, E[a^2], E[b^2], E[ab]; var = E[x^2] - mu^2, cov = E[ab] - mu_a mu_b;
 * C1 = (0.01 peak)^2, C2 = (0.03 peak)^2;
 *     ssim = ((2 mu_a mu_b + C1)(2 cov + C2)) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2))
 * over the windows that lie wholly inside the raster.
 *
 * SAM (what & LBDRN_QUALITY_SAM, 2 <= C <= 16; otherwise sam_n = 0), over the C samples of a pixel:
 *     dot = sum a_c b_c (exact), cross = sum over i < j of (a_i b_j - a_j b_i)^2 (each difference the exact integer -- it
 *     is below 2^33 in magnitude, so float64 forms it without rounding --, the squares summed in float64 in the order i,
 *     then j), theta = atan2(sqrt(cross), dot) in radians.
 * A pixel with a = 0 in every band, or b = 0 in every band, is counted in sam_undefined; with both, theta = 0.
 *
 * Determinism: the integer fields are integer atomics; the float64 sums are per-workgroup partial sums in the workspace,
 * added by a last launch in a fixed order; the cut into workgroups depends on (C, H, W) alone (4 rows of all bands per
 * statistics workgroup, 32 x 32 windows per SSIM workgroup).  A result is bit-identical from run to run, stream to stream
 * and device to device.
 *
 * Conventions are those of lbdrn_resid.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_quality_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); the call
 * enqueues on it and does not synchronise.  The workspace's contents do not matter on entry, nothing beyond the stated
 * sizes is written, a and b are only read, and every check of the arguments comes before any launch and needs no device.
 *
 *   lbdrn_quality_result_bytes  2112 C + 32 (0: C out of range -- 1 <= C <= 65535)
 *   lbdrn_quality_workspace     device scratch bytes a call with these arguments needs: 8 per statistics workgroup where
 *                               SAM runs, 8 per SSIM tile and band where SSIM runs; may be 0, and is 0 for a geometry out of
 *                               range (1 <= H, W <= 2^20, H * W <= 2^31)
 *   lbdrn_quality_compare       bits: 8 or 16.  LBDRN_E_ARG for a null pointer, bits, a geometry or a stride out of range,
 *                               a peak that is not a positive finite number, unknown bits in `what`, a result that is not
 *                               8-byte aligned; LBDRN_E_WORKSPACE for a short workspace.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_QUALITY_ABI_VERSION 1
#define LBDRN_QUALITY_SSIM 1u
#define LBDRN_QUALITY_SAM 2u

const char *lbdrn_quality_last_error(void);
int lbdrn_quality_abi_version(void);
size_t lbdrn_quality_result_bytes(int32_t C);
size_t lbdrn_quality_workspace(int32_t C, int32_t H, int32_t W, uint32_t what);
int lbdrn_quality_compare(const void *a, int64_t a_row, int64_t a_plane, const void *b, int64_t b_row, int64_t b_plane, int32_t bits,
                          int32_t C, int32_t H, int32_t W, double peak, uint32_t what, void *result, void *workspace,
                          size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
