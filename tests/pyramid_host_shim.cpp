// The host build of the overview pyramid's text: csrc/pyramid.inc compiled by a host compiler behind a few C functions for
// tests/test_pyramid_host.py, tests/test_gpu_pyramid.py (ctypes) and tests/pyramid_main.cpp.  The geometry and the per-sample
// functions are the device's; the loops around them are plain and sequential here.  TEST INFRASTRUCTURE.
#include <stdlib.h>
#include <string.h>

#include "pyramid.inc"

namespace {

template <class T, int RESAMPLING, bool NODATA>
void reduce_level(const T* src, int64_t row, int64_t plane, int C, int Hs, int Ws, T* dst, uint32_t nodata)
{
    const int Hd = pyramid::half_up(Hs), Wd = pyramid::half_up(Ws);
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x)
                dst[((int64_t)c * Hd + y) * Wd + x] = (T)pyramid::reduce_at<T, RESAMPLING, NODATA>(src + c * plane, row, Hs, Ws, y, x, nodata);
}

template <class T>
void build(const T* src, int64_t row, int64_t plane, int C, int H, int W, int resampling, int has_nodata, uint32_t nodata, int levels,
           unsigned char* out)
{
    const T* from = src;
    int Hs = H, Ws = W;
    for (int k = 1; k <= levels; ++k) {
        T* to = (T*)(out + pyramid::level_offset(C, H, W, k, (int)sizeof(T)));
        if (resampling == pyramid::NEAREST) reduce_level<T, pyramid::NEAREST, false>(from, row, plane, C, Hs, Ws, to, nodata);
        else if (has_nodata) reduce_level<T, pyramid::AVERAGE, true>(from, row, plane, C, Hs, Ws, to, nodata);
        else reduce_level<T, pyramid::AVERAGE, false>(from, row, plane, C, Hs, Ws, to, nodata);
        Hs = pyramid::half_up(Hs);
        Ws = pyramid::half_up(Ws);
        from = to;
        row = Ws;
        plane = (int64_t)Hs * Ws;
    }
}

}  // namespace

extern "C" {

int pyr_shim_max_levels(int H, int W) { return pyramid::max_levels(H, W); }
int pyr_shim_level_count(int H, int W, int stop) { return pyramid::auto_levels(H, W, stop); }
void pyr_shim_level_size(int H, int W, int k, int* Hk, int* Wk) { pyramid::level_size(H, W, k, Hk, Wk); }
uint64_t pyr_shim_level_offset(int C, int H, int W, int k, int sample_bytes) { return pyramid::level_offset(C, H, W, k, sample_bytes); }
uint64_t pyr_shim_output_bytes(int C, int H, int W, int levels, int sample_bytes) { return pyramid::output_bytes(C, H, W, levels, sample_bytes); }
uint32_t pyr_shim_rounded_mean(uint32_t s, uint32_t n) { return pyramid::rounded_mean(s, n); }

// the levels 1 .. `levels` of a host raster into out[0 .. output_bytes); the padding between two levels is not written;
// returns 0, or -1 for arguments the library refuses too
int pyr_shim_build(const void* src, int64_t row, int64_t plane, int bits, int C, int H, int W, int resampling, int has_nodata,
                   uint32_t nodata, int levels, void* out)
{
    if (!src || !out || !pyramid::geom_ok(C, H, W) || (bits != 8 && bits != 16) || row < W || plane < 0 || levels < 1 ||
        levels > pyramid::max_levels(H, W) || (resampling != pyramid::AVERAGE && resampling != pyramid::NEAREST) ||
        (has_nodata != 0 && has_nodata != 1) || (has_nodata && nodata >= (1u << bits)))
        return -1;
    if (bits == 8) build<uint8_t>((const uint8_t*)src, row, plane, C, H, W, resampling, has_nodata, nodata, levels, (unsigned char*)out);
    else build<uint16_t>((const uint16_t*)src, row, plane, C, H, W, resampling, has_nodata, nodata, levels, (unsigned char*)out);
    return 0;
}

}  // extern "C"
