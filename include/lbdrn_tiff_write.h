/* liblbdrn_tiffw.so -- the strips and tiles of a TIFF raster built and Deflate-compressed on the GPU (csrc/tiffw.hip,
 * csrc/tiffw.inc), plain C ABI.  The way out of every command line here is raster_io.write_raster; this library is what
 * lets it write tiled, Deflate-compressed, predictor-2 files from planes that already sit in device memory, so that only
 * the compressed bytes are downloaded.  It is the counterpart of liblbdrn_tiff.so (include/lbdrn_tiff.h) and shares its
 * layout description, its segment order and its conventions; the two libraries do not depend on each other.
 *
 * The ABI takes planes and a layout and returns segment bytes and their table, not a file: the host (lbdrn_hip/
 * tiff_write.py) writes the header, the IFD and the tables around them.  A segment is a strip or a tile.  Segments are in
 * TIFF order: tiles left to right, then top to bottom; with planar = 2, all of band 0, then band 1, ...
 *
 * Three stages.
 *   gather     one wave per segment row, the inverse of the reader's placement: planes[C][H][W] -> the segment's byte
 *              image, chunky or planar, little-endian, edge tiles zero-filled to the full tile, predictor 2 applied per
 *              sample channel modulo 2^bits (over the zero fill as well, as libtiff does).  With compression 1 this
 *              stage writes `out` directly.
 *   deflate    one wave per segment, RFC 1950 / 1951: a zlib header, blocks of at most lbdrn_tiffw_block_tokens() LZ77
 *              tokens (greedy matches of 3..258 bytes at distances 1..32768 inside the segment), each block written as a
 *              dynamic, a fixed or stored block(s), whichever is smallest by exact bit count, and the Adler-32.
 *   pack       an exclusive scan of the segments' sizes, and each segment copied to its place in `out`.
 * The bytes are a function of the planes and the layout alone: the same from run to run, on any stream, whatever the
 * workspace and `out` held before.
 *
 * Conventions are those of lbdrn_tiff.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_tiffw_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); the encode
 * call enqueues on it and does not synchronise.  The workspace's contents do not matter on entry, nothing beyond the
 * stated sizes is written, and `planes` is only read.
 *
 *   lbdrn_tiffw_segment_count   segments of the layout; 0: layout out of range (the reader's ranges: C <= 65535, H, W,
 *                               seg_w, seg_h <= 2^20, bits 8 / 16, a strip layout has seg_w = W and seg_h <= H, at most
 *                               2^30 segments; and for this writer big_endian = 0 and compression 1 or 8)
 *   lbdrn_tiffw_segment_cap     the largest uncompressed segment, in bytes, this library writes with that compression (0:
 *                               not a compression of this library).  For Deflate it equals lbdrn_tiff_segment_cap(8), so
 *                               the device reader reads on the device whatever this writer writes.
 *   lbdrn_tiffw_bound           the most bytes a segment of segment_bytes uncompressed bytes takes once Deflate-coded
 *   lbdrn_tiffw_block_tokens    the capacity of the token buffer: a block holds at most that many literals and matches
 *   lbdrn_tiffw_output_bytes    the size `out` must have: every segment at its bound (compression 8) or at its size
 *                               (compression 1); 0: layout out of range
 *   lbdrn_tiffw_workspace       device scratch bytes lbdrn_tiffw_encode needs, a function of the layout alone: one slot per
 *                               segment for its byte image and one for its stream, and the scan's scratch; 0 with
 *                               compression 1 (the gather writes `out`) and for a layout out of range
 *   lbdrn_tiffw_encode          planes: DEVICE [C][H][W], uint8 or uint16 by bits.  out: DEVICE, out_bytes bytes; receives
 *                               the segments back to back in segment order.  offsets, counts: DEVICE, nseg uint64 each,
 *                               8-byte aligned; offsets[s] is relative to `out`.  total: DEVICE, one uint64, the sum of
 *                               counts.  Checked before any launch, in this order: null pointers, the layout's ranges and
 *                               out_bytes < lbdrn_tiffw_output_bytes (LBDRN_E_ARG); the layout's segment size against the
 *                               cap (LBDRN_E_UNSUPPORTED); the workspace (LBDRN_E_WORKSPACE).
 */
#ifndef LBDRN_TIFF_WRITE_H
#define LBDRN_TIFF_WRITE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_TIFFW_ABI_VERSION 1

/* field for field the reader's lbdrn_tiff_layout */
typedef struct lbdrn_tiffw_layout {
    int32_t C, H, W;          /* SamplesPerPixel, ImageLength, ImageWidth */
    int32_t bits;             /* 8 or 16, unsigned integer samples */
    int32_t big_endian;       /* must be 0: little-endian files only */
    int32_t planar;           /* 1 chunky, 2 planar */
    int32_t seg_w, seg_h;     /* tile size; strips: seg_w = W, seg_h = RowsPerStrip */
    int32_t tiled;            /* 0 strips (the last one is short), 1 tiles (always full size in the file, zero-filled) */
    int32_t compression;      /* 1 none, 8 Deflate */
    int32_t predictor;        /* 1 none, 2 horizontal differencing */
} lbdrn_tiffw_layout;

const char *lbdrn_tiffw_last_error(void);
int lbdrn_tiffw_abi_version(void);
size_t lbdrn_tiffw_segment_count(const lbdrn_tiffw_layout *layout);
size_t lbdrn_tiffw_segment_cap(int32_t compression);
size_t lbdrn_tiffw_bound(size_t segment_bytes);
size_t lbdrn_tiffw_block_tokens(void);
size_t lbdrn_tiffw_output_bytes(const lbdrn_tiffw_layout *layout);
size_t lbdrn_tiffw_workspace(const lbdrn_tiffw_layout *layout);
int lbdrn_tiffw_encode(const lbdrn_tiffw_layout *layout, const void *planes, void *out, size_t out_bytes, uint64_t *offsets,
                       uint64_t *counts, uint64_t *total, void *workspace, size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
