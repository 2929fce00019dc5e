// liblbdrn_tiff.so (include/lbdrn_tiff.h): the strips and tiles of a TIFF scene, decompressed and placed on the GPU.  The
// format's text (segment geometry, Deflate, TIFF LZW, PackBits) is csrc/tiff.inc, shared with the host tests.
//
//   k_tiff_inflate    one wave per segment, the shape of k_jp2k_unblocks: the bit decoder is wave-uniform (every lane
//   k_tiff_lzw        decodes the same bits), the stream passes through LDS 512 bytes at a time, and the tables are in LDS:
//   k_tiff_packbits   Deflate's 32 KB history ring, its two canonical codes and their fast tables (37 KB a wave); LZW's
//                     4096 entries of (prefix code, last byte, length) (16.5 KB a wave).  The wave shares stored blocks,
//                     matches (byte i of a match is byte i mod distance of the history in front of it, so overlapping
//                     matches need no order among the lanes), PackBits runs and the Adler-32 sums.  An LZW string is a
//                     pointer chase along its prefix chain, which one lane writes.  Each segment goes to its slot of the
//                     workspace; status[s] receives the decoder's verdict.
//   k_tiff_place      one wave per segment row: the row's samples in native byte order, predictor 2 undone by a wave
//                     prefix sum per sample channel (64 samples a step, the carry in the last lane), edge tiles cropped,
//                     and one coalesced store per channel and step into planes[C][H][W].  Uncompressed segments are read
//                     from the file itself; a byte count short of the segment is status 1.
#include <string.h>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_tiff.h"
#include "tiff.inc"

namespace lbdrn {

struct TiffWs {
    uint64_t* offsets;   // [nseg]
    uint64_t* counts;    // [nseg]
    uint8_t* slots;      // [nseg][pitch], compressed layouts only
    size_t total;
};

static void carve_tiff(const tiff::Geom& g, void* ws, TiffWs* w)
{
    char* p = (char*)ws;
    w->offsets = (uint64_t*)p; p += align_up((size_t)g.nseg * 8, 256);
    w->counts = (uint64_t*)p; p += align_up((size_t)g.nseg * 8, 256);
    w->slots = (uint8_t*)p;
    if (g.compression != tiff::COMP_NONE) p += align_up((size_t)g.nseg * (size_t)g.pitch, 256);
    w->total = (size_t)(p - (char*)ws);
}

// ------------------------------------------------------------------ decompression: one wave per segment

__global__ void __launch_bounds__(64) k_tiff_inflate(const uint8_t* __restrict__ file, const uint64_t* __restrict__ offsets,
                                                      const uint64_t* __restrict__ counts, tiff::Geom g, uint8_t* __restrict__ slots,
                                                      int32_t* __restrict__ status)
{
    __shared__ tiff::InflateTables t;
    const int64_t s = blockIdx.x;
    const int st = tiff::inflate(file + offsets[s], (size_t)counts[s], slots + (size_t)s * (size_t)g.pitch, (size_t)tiff::seg_expected(g, s),
                                 &t, (int)threadIdx.x, 64);
    if (threadIdx.x == 0) status[s] = st;
}

__global__ void __launch_bounds__(64) k_tiff_lzw(const uint8_t* __restrict__ file, const uint64_t* __restrict__ offsets,
                                                  const uint64_t* __restrict__ counts, tiff::Geom g, uint8_t* __restrict__ slots,
                                                  int32_t* __restrict__ status)
{
    __shared__ tiff::LzwTables t;
    const int64_t s = blockIdx.x;
    const int st = tiff::lzw(file + offsets[s], (size_t)counts[s], slots + (size_t)s * (size_t)g.pitch, (size_t)tiff::seg_expected(g, s),
                             &t, (int)threadIdx.x, 64);
    if (threadIdx.x == 0) status[s] = st;
}

__global__ void __launch_bounds__(64) k_tiff_packbits(const uint8_t* __restrict__ file, const uint64_t* __restrict__ offsets,
                                                       const uint64_t* __restrict__ counts, tiff::Geom g, uint8_t* __restrict__ slots,
                                                       int32_t* __restrict__ status)
{
    __shared__ tiff::PackBitsTables t;
    const int64_t s = blockIdx.x;
    const int st = tiff::packbits(file + offsets[s], (size_t)counts[s], slots + (size_t)s * (size_t)g.pitch,
                                  (size_t)tiff::seg_expected(g, s), &t, (int)threadIdx.x, 64);
    if (threadIdx.x == 0) status[s] = st;
}

// ------------------------------------------------------------------ placement: one wave per segment row

template <typename T>
__global__ void __launch_bounds__(64) k_tiff_place(const uint8_t* __restrict__ file, const uint64_t* __restrict__ offsets,
                                                    const uint64_t* __restrict__ counts, tiff::Geom g, const uint8_t* __restrict__ slots,
                                                    T* __restrict__ planes, int32_t* __restrict__ status)
{
    const int lane = threadIdx.x;
    const int64_t s = (int64_t)(blockIdx.x / (unsigned)g.seg_h);
    const int r = (int)(blockIdx.x % (unsigned)g.seg_h);
    const uint8_t* src;
    if (g.compression == tiff::COMP_NONE) {
        if (counts[s] < (uint64_t)tiff::seg_expected(g, s)) {      // (offset + count lies inside the file: the host checked)
            if (r == 0 && lane == 0) status[s] = tiff::ST_TRUNCATED;
            return;
        }
        src = file + offsets[s];
    } else {
        src = slots + (size_t)s * (size_t)g.pitch;
    }
    if (r >= tiff::seg_rows(g, s)) return;
    src += (size_t)r * (size_t)g.row_bytes;
    const int64_t t = s % g.per_plane;
    const int x0 = (int)(t % g.segs_x) * g.seg_w, y = (int)(t / g.segs_x) * g.seg_h + r;
    const int cols = min(g.seg_w, g.W - x0);
    for (int ch = 0; ch < g.spp; ++ch) {
        const int c = g.spp == 1 ? (int)(s / g.per_plane) : ch;
        T* dst = planes + ((size_t)c * g.H + (size_t)y) * g.W + x0;
        uint32_t carry = 0;
        for (int xb = 0; xb < cols; xb += 64) {
            const int x = xb + lane;
            uint32_t v = 0;
            if (x < cols) {
                const uint8_t* q = src + ((size_t)x * g.spp + ch) * sizeof(T);
                if (sizeof(T) == 1) v = q[0];
                else v = g.big_endian ? ((uint32_t)q[0] << 8) | q[1] : ((uint32_t)q[1] << 8) | q[0];
            }
            if (g.predictor == 2) {      // sums modulo 2^bits: the low bits of 32-bit sums
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(v, o, 64);
                    if (lane >= o) v += up;
                }
                v += carry;
                carry = __shfl(v, 63, 64);
            }
            if (x < cols) dst[x] = (T)v;
        }
    }
}

// ------------------------------------------------------------------ host entry point

static int tiff_decode(const lbdrn_tiff_layout* L, const void* file, size_t file_bytes, const uint64_t* offsets, const uint64_t* counts,
                       size_t nseg, void* planes, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(L && file && offsets && counts && planes && status, "lbdrn_tiff_decode: null pointer");
    LBDRN_REQUIRE(((uintptr_t)status & 3u) == 0, "lbdrn_tiff_decode: status is not 4-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)ws & 255u) == 0, "lbdrn_tiff_decode: workspace is not 256-byte aligned");   // (carve_tiff: u64 regions at multiples of 256)
    tiff::Geom g;
    LBDRN_REQUIRE(tiff::make_geom(*L, &g), "lbdrn_tiff_decode: the layout is out of range");
    LBDRN_REQUIRE((int64_t)nseg == g.nseg, "lbdrn_tiff_decode: %zu segments given, the layout has %lld", nseg, (long long)g.nseg);
    for (size_t i = 0; i < nseg; ++i)
        LBDRN_REQUIRE(offsets[i] <= file_bytes && counts[i] <= file_bytes - offsets[i],
                      "lbdrn_tiff_decode: segment %zu (offset %llu, %llu bytes) does not lie inside the file's %zu bytes", i,
                      (unsigned long long)offsets[i], (unsigned long long)counts[i], file_bytes);
    if ((uint64_t)g.seg_bytes > (uint64_t)tiff::segment_cap(g.compression)) {
        set_error("lbdrn_tiff_decode: a segment of %lld bytes is above the cap of %zu bytes for compression %d", (long long)g.seg_bytes,
                  tiff::segment_cap(g.compression), g.compression);
        return LBDRN_E_UNSUPPORTED;
    }
    LBDRN_REQUIRE(g.bps == 1 || ((uintptr_t)planes & 1u) == 0, "lbdrn_tiff_decode: planes is not 2-byte aligned");   // (16-bit samples)
    TiffWs w;
    carve_tiff(g, ws, &w);
    if (!ws || ws_bytes < w.total) {
        set_error("TIFF reader workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    LBDRN_HIP_TRY(hipMemcpyAsync(w.offsets, offsets, nseg * 8, hipMemcpyHostToDevice, s));
    LBDRN_HIP_TRY(hipMemcpyAsync(w.counts, counts, nseg * 8, hipMemcpyHostToDevice, s));
    LBDRN_HIP_TRY(hipMemsetAsync(status, 0, nseg * sizeof(int32_t), s));
    const uint8_t* f = (const uint8_t*)file;
    if (g.compression == tiff::COMP_DEFLATE) k_tiff_inflate<<<(unsigned)nseg, 64, 0, s>>>(f, w.offsets, w.counts, g, w.slots, status);
    else if (g.compression == tiff::COMP_LZW) k_tiff_lzw<<<(unsigned)nseg, 64, 0, s>>>(f, w.offsets, w.counts, g, w.slots, status);
    else if (g.compression == tiff::COMP_PACKBITS) k_tiff_packbits<<<(unsigned)nseg, 64, 0, s>>>(f, w.offsets, w.counts, g, w.slots, status);
    LBDRN_LAUNCH_CHECK();
    const unsigned rows = (unsigned)(g.nseg * g.seg_h);      // < 2^31: make_geom
    if (g.bps == 1) k_tiff_place<uint8_t><<<rows, 64, 0, s>>>(f, w.offsets, w.counts, g, w.slots, (uint8_t*)planes, status);
    else k_tiff_place<uint16_t><<<rows, 64, 0, s>>>(f, w.offsets, w.counts, g, w.slots, (uint16_t*)planes, status);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_tiff_last_error(void) { return lbdrn::last_error(); }
int lbdrn_tiff_abi_version(void) { return LBDRN_TIFF_ABI_VERSION; }

size_t lbdrn_tiff_segment_count(const lbdrn_tiff_layout* layout)
{
    tiff::Geom g;
    return layout && tiff::make_geom(*layout, &g) ? (size_t)g.nseg : 0;
}

size_t lbdrn_tiff_segment_cap(int32_t compression) { return tiff::segment_cap(compression); }

size_t lbdrn_tiff_workspace(const lbdrn_tiff_layout* layout)
{
    tiff::Geom g;
    lbdrn::TiffWs w;
    if (!layout || !tiff::make_geom(*layout, &g)) return 0;
    lbdrn::carve_tiff(g, nullptr, &w);
    return w.total;
}

int lbdrn_tiff_decode(const lbdrn_tiff_layout* layout, const void* file, size_t file_bytes, const uint64_t* offsets, const uint64_t* counts,
                      size_t nseg, void* planes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::tiff_decode(layout, file, file_bytes, offsets, counts, nseg, planes, status, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
