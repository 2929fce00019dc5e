/* liblbdrn_tiff.so -- the segments of a TIFF scene decompressed and placed on the GPU (csrc/tiff.hip, csrc/tiff.inc), plain
 * C ABI.  The front door of every command line here is raster_io.read_raster; this library is what lets it read the files
 * GDAL's GTiff driver writes with TILED=YES, COMPRESS=LZW / DEFLATE / PACKBITS, PREDICTOR=2 and BIGTIFF=YES.
 *
 * The ABI takes a parsed layout, not a file: the host (lbdrn_hip/tiff.py) reads the IFD and hands over the geometry, the
 * whole file in device memory, and the table of segment offsets and byte counts.  A segment is a strip or a tile.
 * Segments are in TIFF order: tiles left to right, then top to bottom; with planar = 2, all of band 0, then band 1, ...
 *
 * Two stages.  Decompression: one kernel per codec, one wave per segment, each segment into its slot of the workspace
 *   Deflate    RFC 1950 / 1951: the zlib wrapper, stored, fixed and dynamic blocks, any number of blocks, Adler-32 checked
 *   LZW        TIFF 6.0: MSB-first codes of 9..12 bits, Clear 256, EOI 257, early change
 *   PackBits
 * (uncompressed segments are read where they lie).  Placement, k_tiff_place, per segment row: byte order, predictor 2
 * undone per sample channel modulo 2^bits on native-order samples, chunky -> planar, edge tiles cropped, coalesced stores
 * into planes[C][H][W].
 *
 * Conventions are those of lbdrn_resid.h: every call returns 0 or a negative lbdrn_status (the values of lbdrn_hip.h),
 * lbdrn_tiff_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  `stream` is a hipStream_t passed as void* (NULL = default stream); the decode
 * call enqueues on it and does not synchronise.  The workspace's contents do not matter on entry, nothing beyond the
 * stated sizes is written, and a short workspace is LBDRN_E_WORKSPACE before any launch.
 * Alignment (LBDRN_E_ARG before any launch otherwise): the workspace 256 bytes -- its segment table is 64-bit words at
 * the base --, status 4, planes of 16-bit samples 2.  The file needs none: it is read bytewise.
 *
 *   lbdrn_tiff_segment_count  segments of the layout; 0: layout out of range (C <= 65535, H, W, seg_w, seg_h <= 2^20,
 *                             bits 8 / 16, a strip layout has seg_w = W and seg_h <= H, at most 2^30 segments)
 *   lbdrn_tiff_segment_cap    the largest uncompressed segment, in bytes, the device decodes for this compression (0:
 *                             not a compression of this library).  A serial stream is one wave's work; the cap keeps
 *                             the longest one near a quarter of a second.
 *   lbdrn_tiff_workspace      device scratch bytes lbdrn_tiff_decode needs: the segment table, and one slot per segment
 *                             where the layout is compressed
 *   lbdrn_tiff_decode         file: DEVICE, the file's bytes.  offsets, counts: HOST, nseg entries each; they are copied
 *                             to the workspace on `stream` and must stay valid until that copy has run.  Validated before any launch: nseg against the layout (LBDRN_E_ARG), every
 *                             offset + count inside file_bytes (LBDRN_E_ARG), the layout's segment size against the cap
 *                             (LBDRN_E_UNSUPPORTED), the workspace (LBDRN_E_WORKSPACE).  planes: DEVICE [C][H][W], uint8 or
 *                             uint16 by bits.  status: DEVICE [nseg] int32; status[s] is set to 0 and then to non-zero
 *                             where segment s is damaged: the stream ends before the segment's expected size is produced
 *                             (1), a Huffman code, block header, LZW code or PackBits run is invalid (2), a match distance
 *                             points before the segment's start (3), the zlib header is bad (4), the Adler-32 is wrong
 *                             (5).  Decoding stops at the expected size.  A damaged segment gives unspecified samples in
 *                             its own rectangle; it never causes an access outside file, the workspace, planes or status,
 *                             and no decoder loop runs without consuming input or producing output.
 */
#ifndef LBDRN_TIFF_H
#define LBDRN_TIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_TIFF_ABI_VERSION 1

typedef struct lbdrn_tiff_layout {
    int32_t C, H, W;          /* SamplesPerPixel, ImageLength, ImageWidth */
    int32_t bits;             /* 8 or 16, unsigned integer samples */
    int32_t big_endian;       /* byte order of 16-bit samples in the file */
    int32_t planar;           /* 1 chunky, 2 planar */
    int32_t seg_w, seg_h;     /* tile size; strips: seg_w = W, seg_h = RowsPerStrip */
    int32_t tiled;            /* 0 strips (the last one may be short), 1 tiles (always full size in the file, cropped on placement) */
    int32_t compression;      /* 1 none, 5 LZW, 8 Deflate (32946 is handed over as 8), 32773 PackBits */
    int32_t predictor;        /* 1 none, 2 horizontal differencing */
} lbdrn_tiff_layout;

const char *lbdrn_tiff_last_error(void);
int lbdrn_tiff_abi_version(void);
size_t lbdrn_tiff_segment_count(const lbdrn_tiff_layout *layout);
size_t lbdrn_tiff_segment_cap(int32_t compression);
size_t lbdrn_tiff_workspace(const lbdrn_tiff_layout *layout);
int lbdrn_tiff_decode(const lbdrn_tiff_layout *layout, const void *file, size_t file_bytes, const uint64_t *offsets,
                      const uint64_t *counts, size_t nseg, void *planes, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
