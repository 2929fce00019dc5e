/* liblbdrn_jp2k_dec.so -- the GPU decoder of the lossless JPEG 2000 MSB payload (csrc/jp2k_dec.hip), plain C ABI.
 *
 * Reads what lbdrn_jp2k_encode (include/lbdrn_hip.h) writes and what OpenJPEG (this package's liblbdrn_jp2.so) and Pillow
 * write with reversible settings, without OpenJPEG: the host parses boxes, headers and packet headers into a validated
 * table of code blocks, the device decodes the blocks (T.800 Annexes C, D), undoes the 5/3 wavelet (Annex F), the
 * reversible component transform where the file has one (G.2) and the DC shift, and leaves the planes in HBM, as
 * lbdrn_plane_decode leaves LBB2's.
 *
 * Accepted: a .jp2 file or a raw codestream with unsigned components of one depth of 1..16 bits, all of the image's size,
 * any tile size, reversible 5/3 with 0..16 decompositions, no component transform or the reversible one (RCT; on
 * components 0 - 2 of three or more), one quality layer, LRCP, code blocks up to 64 x 64 of style 0, default precincts or
 * a precinct partition (one size per resolution in COD, down to exponent 0 at the lowest resolution; at most 2^20
 * precincts per resolution of a tile), no quantisation, SOP / EPH present or absent, several tile-parts per tile,
 * COM / TLM / PLT / PLM / CRG segments (skipped).  Anything else -- 9/7, several layers, other progression orders, other
 * block styles, the component transform on fewer than three components, signed or sub-sampled components, PPM / PPT,
 * COC / QCC / RGN / POC -- is LBDRN_E_UNSUPPORTED with a message that names the feature, before anything is launched.
 *
 * Conventions are those of lbdrn_hip.h: every call returns 0 or a negative lbdrn_status (the same values),
 * lbdrn_jp2kd_last_error() returns a per-thread message for the last failure, the library reads no environment variable
 * and keeps no state besides that message.  A damaged or truncated file is LBDRN_E_ARG, or a raster of unspecified
 * values; it is never an access outside `buf`, the planes or the workspace.
 *
 *   lbdrn_jp2kd_info       host only, needs no device: validates the whole file (headers and every packet header) and
 *                          returns its geometry; `bits` is the components' precision
 *   lbdrn_jp2kd_workspace  device scratch bytes for this file (host only); 0 for a file that is refused
 *   lbdrn_jp2kd_decode     buf is HOST memory (n bytes), planes DEVICE memory [C][H][W] uint16; C, H, W must be the file's.
 *                          The workspace's contents do not matter on entry, nothing beyond workspace_bytes is touched, and
 *                          a workspace shorter than lbdrn_jp2kd_workspace(buf, n) is LBDRN_E_WORKSPACE before any launch.
 *                          Alignment (LBDRN_E_ARG before any launch otherwise): the workspace 256 bytes (32-bit words from
 *                          its base), planes 2; buf is read bytewise and needs none.
 *                          Runs on `stream` (a hipStream_t passed as void*; NULL = default stream) and synchronises it.
 */
#ifndef LBDRN_JP2K_DEC_H
#define LBDRN_JP2K_DEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LBDRN_JP2KD_ABI_VERSION 1

const char *lbdrn_jp2kd_last_error(void);
int lbdrn_jp2kd_abi_version(void);
int lbdrn_jp2kd_info(const void *buf, size_t n, int32_t *C, int32_t *H, int32_t *W, int32_t *bits);
size_t lbdrn_jp2kd_workspace(const void *buf, size_t n);
int lbdrn_jp2kd_decode(const void *buf, size_t n, uint16_t *planes, int32_t C, int32_t H, int32_t W, void *workspace,
                       size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
