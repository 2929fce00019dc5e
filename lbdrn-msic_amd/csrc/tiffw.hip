// liblbdrn_tiffw.so (include/lbdrn_tiff_write.h): the strips and tiles of a TIFF raster built and Deflate-compressed on the
// GPU.  The format's text (gather of a segment row, the Deflate encoder) is csrc/tiffw.inc, shared with the host tests.
//
//   k_tiffw_gather    one wave per segment row, the inverse of k_tiff_place: one coalesced load per channel and step from
//                     planes[C][H][W], zero outside the image, predictor 2 as the difference to the lane before (the carry
//                     in the last lane), little-endian samples into the segment's byte image -- its slot of the workspace,
//                     or its place in `out` where nothing is compressed.  Row 0 of an uncompressed segment writes the
//                     segment's table entry.
//   k_tiffw_deflate   one wave per segment, all state in LDS (tiffw::DeflateState, 74 KB: two waves on a compute unit): the
//                     segment passes through a 36 KiB ring, each lane hashes and measures one position of a 64-position step, greedy selection is
//                     wave-uniform, and a full token buffer is closed as a block: histograms by LDS atomic adds, code
//                     lengths, the three costs, then 64 tokens a step through a prefix sum of their bit lengths into LDS
//                     words and from there to the segment's output slot.  counts[s] receives the stream's size.
//   k_tiffw_pack      after rocprim's exclusive scan of counts into offsets: each slot copied to its place, and the total.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_tiff_write.h"
#include "tiffw.inc"

namespace lbdrn {

struct TiffwWs {
    uint8_t* raw;        // [nseg][pitch]: the segments' byte images
    uint8_t* coded;      // [nseg][opitch]: their zlib streams
    void* scan_tmp;
    size_t scan_bytes;
    size_t opitch;
    size_t total;
};

// rocprim is asked for its scratch size where it runs, on a device; the workspace reserves this much for it whatever it
// answers, so that the size of the workspace is a function of the layout alone and is known without a device.  (Its
// look-back scan keeps some twenty bytes per block of a thousand or more items: 4 bytes an item and 64 KiB are far above.)
static size_t scan_reserve(const tiff::Geom& g) { return align_up((size_t)65536 + (size_t)g.nseg * 4, 256); }

// (compression 1 needs no workspace: the gather writes `out`)
static void carve_tiffw(const tiff::Geom& g, void* ws, TiffwWs* w)
{
    char* p = (char*)ws;
    w->opitch = align_up(tiffw::bound((size_t)g.seg_bytes), 16);
    w->scan_bytes = 0;
    w->raw = w->coded = nullptr;
    w->scan_tmp = nullptr;
    if (g.compression == tiff::COMP_DEFLATE) {
        w->raw = (uint8_t*)p; p += align_up((size_t)g.nseg * (size_t)g.pitch, 256);
        w->coded = (uint8_t*)p; p += align_up((size_t)g.nseg * w->opitch, 256);
        w->scan_tmp = p; p += scan_reserve(g);
        w->scan_bytes = scan_reserve(g);
    }
    w->total = (size_t)(p - (char*)ws);
}

static size_t output_bytes(const tiff::Geom& g)
{
    if (g.compression == tiff::COMP_NONE) return (size_t)tiffw::plain_offset(g, g.nseg);
    size_t n = 0;      // a plane's last strip is short: segments of two sizes at most
    const int64_t last = tiff::seg_expected(g, g.per_plane - 1);
    const int64_t planes = g.nseg / g.per_plane;
    n += (size_t)(planes * (g.per_plane - 1)) * tiffw::bound((size_t)g.seg_bytes);
    n += (size_t)planes * tiffw::bound((size_t)last);
    return n;
}

template <typename T>
__global__ void __launch_bounds__(64) k_tiffw_gather(const T* __restrict__ planes, tiff::Geom g, uint8_t* __restrict__ slots,
                                                      uint8_t* __restrict__ out, uint64_t* __restrict__ offsets,
                                                      uint64_t* __restrict__ counts, uint64_t* __restrict__ total)
{
    const int lane = threadIdx.x;
    const int64_t s = (int64_t)(blockIdx.x / (unsigned)g.seg_h);
    const int r = (int)(blockIdx.x % (unsigned)g.seg_h);
    uint8_t* seg;
    if (g.compression == tiff::COMP_NONE) {
        const int64_t at = tiffw::plain_offset(g, s);
        seg = out + at;
        if (r == 0 && lane == 0) {
            offsets[s] = (uint64_t)at;
            counts[s] = (uint64_t)tiff::seg_expected(g, s);
            if (s == 0) *total = (uint64_t)tiffw::plain_offset(g, g.nseg);
        }
    } else {
        seg = slots + (size_t)s * (size_t)g.pitch;
    }
    tiffw::gather_row<T>(g, planes, s, r, seg, lane);
}

__global__ void __launch_bounds__(64) k_tiffw_deflate(const uint8_t* __restrict__ slots, tiff::Geom g, uint8_t* __restrict__ coded,
                                                       size_t opitch, uint64_t* __restrict__ counts)
{
    __shared__ tiffw::DeflateState st;
    const int64_t s = blockIdx.x;
    const size_t n = (size_t)tiff::seg_expected(g, s);
    const size_t got = tiffw::deflate(slots + (size_t)s * (size_t)g.pitch, n, coded + (size_t)s * opitch, tiffw::bound(n), &st,
                                      (int)threadIdx.x, 64);
    if (threadIdx.x == 0) counts[s] = (uint64_t)got;
}

__global__ void __launch_bounds__(256) k_tiffw_pack(const uint8_t* __restrict__ coded, size_t opitch, int64_t nseg,
                                                     const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ counts,
                                                     uint8_t* __restrict__ out, size_t out_bytes, uint64_t* __restrict__ total)
{
    const int64_t s = blockIdx.x;
    const uint64_t at = offsets[s], n = counts[s];
    const uint8_t* src = coded + (size_t)s * opitch;
    for (uint64_t i = threadIdx.x; i < n; i += 256)
        if (at + i < (uint64_t)out_bytes) out[at + i] = src[i];
    if (s == nseg - 1 && threadIdx.x == 0) *total = at + n;
}

static int tiffw_encode(const lbdrn_tiffw_layout* L, const void* planes, void* out, size_t out_bytes, uint64_t* offsets, uint64_t* counts,
                        uint64_t* total, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(L && planes && out && offsets && counts && total, "lbdrn_tiffw_encode: null pointer");
    tiff::Geom g;
    LBDRN_REQUIRE(tiffw::make_geom(*L, &g), "lbdrn_tiffw_encode: the layout is out of range");
    LBDRN_REQUIRE(out_bytes >= output_bytes(g), "lbdrn_tiffw_encode: out holds %zu bytes, the layout needs %zu", out_bytes, output_bytes(g));
    if ((uint64_t)g.seg_bytes > (uint64_t)tiffw::segment_cap(g.compression)) {
        set_error("lbdrn_tiffw_encode: a segment of %lld bytes is above the cap of %zu bytes for compression %d", (long long)g.seg_bytes,
                  tiffw::segment_cap(g.compression), g.compression);
        return LBDRN_E_UNSUPPORTED;
    }
    TiffwWs w;
    carve_tiffw(g, ws, &w);
    if (w.total && (!ws || ws_bytes < w.total)) {
        set_error("TIFF writer workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    size_t scan_bytes = 0;
    if (g.compression == tiff::COMP_DEFLATE) {      // (a size query: nothing is launched)
        LBDRN_HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (const uint64_t*)counts, offsets, (uint64_t)0, (size_t)g.nseg,
                                              rocprim::plus<uint64_t>(), s));
        if (scan_bytes > w.scan_bytes) {
            set_error("lbdrn_tiffw_encode: rocprim's scan wants %zu bytes of scratch, %zu are reserved", scan_bytes, w.scan_bytes);
            return LBDRN_E_DEVICE;
        }
    }
    const unsigned rows = (unsigned)(g.nseg * g.seg_h);      // < 2^31: make_geom
    if (g.bps == 1) k_tiffw_gather<uint8_t><<<rows, 64, 0, s>>>((const uint8_t*)planes, g, w.raw, (uint8_t*)out, offsets, counts, total);
    else k_tiffw_gather<uint16_t><<<rows, 64, 0, s>>>((const uint16_t*)planes, g, w.raw, (uint8_t*)out, offsets, counts, total);
    LBDRN_LAUNCH_CHECK();
    if (g.compression == tiff::COMP_NONE) return 0;
    k_tiffw_deflate<<<(unsigned)g.nseg, 64, 0, s>>>(w.raw, g, w.coded, w.opitch, counts);
    LBDRN_LAUNCH_CHECK();
    LBDRN_HIP_TRY(rocprim::exclusive_scan(w.scan_tmp, scan_bytes, (const uint64_t*)counts, offsets, (uint64_t)0, (size_t)g.nseg,
                                          rocprim::plus<uint64_t>(), s));
    k_tiffw_pack<<<(unsigned)g.nseg, 256, 0, s>>>(w.coded, w.opitch, g.nseg, offsets, counts, (uint8_t*)out, out_bytes, total);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_tiffw_last_error(void) { return lbdrn::last_error(); }
int lbdrn_tiffw_abi_version(void) { return LBDRN_TIFFW_ABI_VERSION; }

size_t lbdrn_tiffw_segment_count(const lbdrn_tiffw_layout* layout)
{
    tiff::Geom g;
    return layout && tiffw::make_geom(*layout, &g) ? (size_t)g.nseg : 0;
}

size_t lbdrn_tiffw_segment_cap(int32_t compression) { return tiffw::segment_cap(compression); }
size_t lbdrn_tiffw_bound(size_t segment_bytes) { return tiffw::bound(segment_bytes); }
size_t lbdrn_tiffw_block_tokens(void) { return (size_t)tiffw::TOKCAP; }

size_t lbdrn_tiffw_output_bytes(const lbdrn_tiffw_layout* layout)
{
    tiff::Geom g;
    return layout && tiffw::make_geom(*layout, &g) ? lbdrn::output_bytes(g) : 0;
}

size_t lbdrn_tiffw_workspace(const lbdrn_tiffw_layout* layout)
{
    tiff::Geom g;
    lbdrn::TiffwWs w;
    if (!layout || !tiffw::make_geom(*layout, &g)) return 0;
    lbdrn::carve_tiffw(g, nullptr, &w);
    return w.total;
}

int lbdrn_tiffw_encode(const lbdrn_tiffw_layout* layout, const void* planes, void* out, size_t out_bytes, uint64_t* offsets, uint64_t* counts,
                       uint64_t* total, void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::tiffw_encode(layout, planes, out, out_bytes, offsets, counts, total, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
