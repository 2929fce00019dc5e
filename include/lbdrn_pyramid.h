/* liblbdrn_pyramid.so -- the overview levels of a raster that lies in HBM, reduced on the GPU (csrc/pyramid.hip,
 * csrc/pyramid.inc), plain C ABI.
 *
 * Geometry.  Level 0 is the raster, C planes of H rows and W samples of unsigned 8 or 16 bits.  Level k >= 1 has
 * H_k = ceil(H_{k-1} / 2) rows and W_k = ceil(W_{k-1} / 2) samples, and is computed FROM LEVEL k - 1 (a cascade).  A level
 * whose source is 1 x 1 does not exist: a raster has at most ceil(log2(max(H, W))) levels.
 *
 * The automatic level count (lbdrn_pyr_level_count): level k is written as long as max(H_{k-1}, W_{k-1}) > stop, so the last
 * level fits a square of `stop` samples (a tile).  6000 x 6000 with stop = 256: 5 levels -- 3000, 1500, 750, 375, 188.
 *
 * LBDRN_PYR_AVERAGE.  Output (y, x) takes the source samples (2y + dy, 2x + dx), dy, dx in {0, 1}, that lie inside level
 * k - 1; with has_nodata, only those whose value differs from nodata.  With n such samples and sum s the result is
 * (s + n / 2) / n in integers (round half up; s is formed in 32 bits); n is 1, 2 or 4, with nodata also 3; n = 0 gives
 * nodata.  A valid average that happens to equal nodata is left as it is: the next level then takes it for nodata.
 * LBDRN_PYR_NEAREST.  The source sample (2y, 2x), which is always inside; nodata does not enter.
 *
 * The source is read where it lies: unit sample stride, row_pitch >= W and plane_pitch >= 0 in samples -- a window of a
 * larger scene is such a view.  The output holds the levels 1 .. L back to back, each a contiguous [C][H_k][W_k], each
 * start at a multiple of 256 bytes from `out`; level k >= 2 reads level k - 1 out of `out`.  No workspace.
 *
 * Conventions are those of lbdrn_quality.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_pyr_last_error() returns a per-thread message for the last failure, the library reads no environment variable and
 * keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); lbdrn_pyr_build
 * enqueues one launch per level on it and does not synchronise.  Nothing beyond lbdrn_pyr_output_bytes is written, the
 * padding between two levels included; the source is only read; every check of the arguments comes before any launch and
 * needs no device, in this order:
 *   LBDRN_E_ARG          a null pointer; C, H, W out of range (1 <= C <= 65535, 1 <= H, W <= 2^20, H * W <= 2^31); bits outside
 *                        1 .. 32; pitches below the stated bounds; has_nodata other than 0 / 1; a nodata value the samples
 *                        cannot hold; levels < 1 or above the raster's count; src or out not aligned to a sample; a short out
 *   LBDRN_E_UNSUPPORTED  bits other than 8 and 16; a resampling other than the two above
 *
 *   lbdrn_pyr_level_count   the automatic count (>= 0), or LBDRN_E_ARG for H, W or stop < 1
 *   lbdrn_pyr_level_size    H_k, W_k for k >= 0; LBDRN_E_ARG for a level that does not exist
 *   lbdrn_pyr_level_offset  byte offset of level k (1 <= k <= levels the raster has) in the output; 0 for what is refused
 *   lbdrn_pyr_output_bytes  the end of level `levels`; 0 for what is refused
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

#define LBDRN_PYR_ABI_VERSION 1
#define LBDRN_PYR_AVERAGE 0
#define LBDRN_PYR_NEAREST 1

typedef struct lbdrn_pyr_desc {
    int32_t C, H, W;
    int32_t bits;            /* 8 or 16, unsigned */
    int32_t resampling;      /* LBDRN_PYR_AVERAGE / LBDRN_PYR_NEAREST */
    int32_t has_nodata;      /* 0 / 1 */
    uint32_t nodata;
    int32_t reserved;        /* 0 */
    int64_t row_pitch;       /* of the source, in samples */
    int64_t plane_pitch;
} lbdrn_pyr_desc;

const char *lbdrn_pyr_last_error(void);
int lbdrn_pyr_abi_version(void);
int lbdrn_pyr_level_count(int32_t H, int32_t W, int32_t stop);
int lbdrn_pyr_level_size(int32_t H, int32_t W, int32_t k, int32_t *Hk, int32_t *Wk);
size_t lbdrn_pyr_level_offset(const lbdrn_pyr_desc *desc, int32_t k);
size_t lbdrn_pyr_output_bytes(const lbdrn_pyr_desc *desc, int32_t levels);
int lbdrn_pyr_build(const lbdrn_pyr_desc *desc, const void *src, int32_t levels, void *out, size_t out_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
