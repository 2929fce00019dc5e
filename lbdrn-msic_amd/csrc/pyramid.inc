// The overview pyramid's text, shared by the device (csrc/pyramid.hip) and the host tests (tests/pyramid_host_shim.cpp):
// the level geometry and the output's layout, the footprint of an output sample, the count of the samples that enter, the
// rounded division and the nodata rule.  Every function here is __host__ __device__ and touches nothing but its
// arguments.  Definitions: include/lbdrn_pyramid.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PYRAMID_HD __host__ __device__ inline
#else
#define PYRAMID_HD inline
#endif

namespace pyramid {

constexpr int AVERAGE = 0, NEAREST = 1;
constexpr int MAX_BANDS = 65535, MAX_SIDE = 1 << 20;
constexpr int64_t MAX_PLANE = (int64_t)1 << 31;
constexpr size_t LEVEL_ALIGN = 256;      // bytes: every level of the output starts on a multiple of it

// ---- geometry
PYRAMID_HD int half_up(int n) { return (n + 1) >> 1; }

PYRAMID_HD bool geom_ok(int C, int H, int W)
{
    return C >= 1 && H >= 1 && W >= 1 && C <= MAX_BANDS && H <= MAX_SIDE && W <= MAX_SIDE && (int64_t)H * W <= MAX_PLANE;
}

// the levels a raster has: level k exists while its source is larger than 1 x 1
PYRAMID_HD int max_levels(int H, int W)
{
    int k = 0;
    while (H > 1 || W > 1) { H = half_up(H); W = half_up(W); ++k; }
    return k;
}

// the automatic count: level k is written as long as the longer side of level k - 1 is above `stop`
PYRAMID_HD int auto_levels(int H, int W, int stop)
{
    int k = 0;
    while ((H > W ? H : W) > stop) { H = half_up(H); W = half_up(W); ++k; }
    return k;
}

PYRAMID_HD void level_size(int H, int W, int k, int* Hk, int* Wk)
{
    for (int i = 0; i < k; ++i) { H = half_up(H); W = half_up(W); }
    *Hk = H; *Wk = W;
}

PYRAMID_HD size_t level_bytes(int C, int H, int W, int k, int sample_bytes)
{
    int h, w;
    level_size(H, W, k, &h, &w);
    return (size_t)C * h * w * sample_bytes;
}

// byte offset of level k >= 1 in the output: the levels before it, each padded to LEVEL_ALIGN
PYRAMID_HD size_t level_offset(int C, int H, int W, int k, int sample_bytes)
{
    size_t at = 0;
    for (int i = 1; i < k; ++i) at += (level_bytes(C, H, W, i, sample_bytes) + LEVEL_ALIGN - 1) / LEVEL_ALIGN * LEVEL_ALIGN;
    return at;
}

PYRAMID_HD size_t output_bytes(int C, int H, int W, int levels, int sample_bytes)
{
    return level_offset(C, H, W, levels, sample_bytes) + level_bytes(C, H, W, levels, sample_bytes);
}

// ---- one output sample
// (s + n / 2) / n for the counts that occur, 1 .. 4: round half up
PYRAMID_HD uint32_t rounded_mean(uint32_t s, uint32_t n)
{
    return n == 3u ? (s + 1u) / 3u : (s + (n >> 1)) >> (n >> 1);
}

struct Acc {
    uint32_t s, n;
};

template <bool NODATA>
PYRAMID_HD void acc_add(Acc* a, uint32_t v, bool inside, uint32_t nodata)
{
    const bool take = inside && (!NODATA || v != nodata);
    a->s += take ? v : 0u;
    a->n += take ? 1u : 0u;
}

// The footprint of output (y, x) is the source samples (2y + dy, 2x + dx): v00 is always inside, v01 where has_x1, v10 where
// has_y1, v11 where both.  A sample that is not inside is not looked at, whatever its argument holds.
template <bool NODATA>
PYRAMID_HD uint32_t average(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, bool has_x1, bool has_y1, uint32_t nodata)
{
    Acc a = {0u, 0u};
    acc_add<NODATA>(&a, v00, true, nodata);
    acc_add<NODATA>(&a, v01, has_x1, nodata);
    acc_add<NODATA>(&a, v10, has_y1, nodata);
    acc_add<NODATA>(&a, v11, has_x1 && has_y1, nodata);
    if (NODATA && a.n == 0u) return nodata;
    return rounded_mean(a.s, a.n);      // (a valid average that equals nodata is left as it is)
}

// output (y, x) of a level from its source plane (Hs rows of Ws samples, `row` samples apart), sample by sample
template <class T, int RESAMPLING, bool NODATA>
PYRAMID_HD uint32_t reduce_at(const T* src, int64_t row, int Hs, int Ws, int y, int x, uint32_t nodata)
{
    const T* p = src + (int64_t)(2 * y) * row + 2 * x;
    if (RESAMPLING == NEAREST) return (uint32_t)p[0];
    const bool has_x1 = 2 * x + 1 < Ws, has_y1 = 2 * y + 1 < Hs;
    const uint32_t v00 = p[0], v01 = has_x1 ? (uint32_t)p[1] : 0u;
    const uint32_t v10 = has_y1 ? (uint32_t)p[row] : 0u, v11 = has_x1 && has_y1 ? (uint32_t)p[row + 1] : 0u;
    return average<NODATA>(v00, v01, v10, v11, has_x1, has_y1, nodata);
}

}  // namespace pyramid
