// liblbdrn_pyramid.so (include/lbdrn_pyramid.h): the overview levels of a raster in HBM, each level reduced 2 x 2 from the
// one before it.  The per-sample text -- footprint, count, rounded division, nodata rule -- is csrc/pyramid.inc, shared with
// the host tests.
//
//   k_pyr_reduce   one launch per level, blockIdx.y the plane.  A lane takes 16 bytes of two source rows (one row for
//                  nearest, and where the second row lies outside) and stores the 8 bytes they reduce to: 4 samples of 16
//                  bits, 8 samples of 8 bits.  Consecutive lanes take consecutive vectors of a row, so a wave reads and
//                  writes contiguous runs.  The vector path needs the 16 source bytes inside the row, both source
//                  addresses on 16 bytes and the destination on 8; a lane for which one of them fails -- a row's tail, an
//                  odd width, a window of a scene -- goes sample by sample through pyramid::reduce_at, which reads nothing
//                  outside the level.  No LDS, no workspace; level k reads level k - 1 out of the output of the launch before.
#include <string.h>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_pyramid.h"
#include "pyramid.inc"

namespace lbdrn {

constexpr int PT = 256;      // threads of a workgroup

template <class T>
__device__ __forceinline__ uint32_t vec_get(const uint4& v, int k)      // (k is a constant after unrolling)
{
    constexpr int per = 4 / (int)sizeof(T), bits = 8 * (int)sizeof(T);
    const uint32_t w = k / per == 0 ? v.x : k / per == 1 ? v.y : k / per == 2 ? v.z : v.w;
    return (w >> (bits * (k % per))) & ((1u << bits) - 1u);
}

template <class T, int RESAMPLING, bool NODATA>
__global__ void __launch_bounds__(PT) k_pyr_reduce(const T* __restrict__ src, int64_t row, int64_t plane, int Hs, int Ws,
                                                    T* __restrict__ dst, int Hd, int Wd, int vpr, uint32_t nodata)
{
    constexpr int N = 16 / (int)sizeof(T), M = N / 2;      // source samples of a vector, output samples they give
    constexpr int per = 4 / (int)sizeof(T), bits = 8 * (int)sizeof(T);
    const int64_t q = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (q >= (int64_t)Hd * vpr) return;
    const int c = (int)blockIdx.y;
    const int y = (int)(q / vpr);
    const int x0 = (int)(q - (int64_t)y * vpr) * M;
    const T* sp = src + (int64_t)c * plane;
    const bool has_y1 = 2 * y + 1 < Hs;
    const T* p0 = sp + (int64_t)(2 * y) * row + 2 * x0;
    const T* p1 = has_y1 && RESAMPLING == pyramid::AVERAGE ? p0 + row : p0;
    T* d = dst + ((int64_t)c * Hd + y) * Wd + x0;
    const bool vec = 2 * x0 + N <= Ws && (((uintptr_t)p0 | (uintptr_t)p1) & 15u) == 0 && ((uintptr_t)d & 7u) == 0;
    if (vec) {
        const uint4 a = *reinterpret_cast<const uint4*>(p0);
        uint32_t o[2] = {0u, 0u};
        if (RESAMPLING == pyramid::NEAREST) {
#pragma unroll
            for (int k = 0; k < M; ++k) o[k / per] |= vec_get<T>(a, 2 * k) << (bits * (k % per));
        } else {
            const uint4 b = *reinterpret_cast<const uint4*>(p1);      // (the first row again where the second lies outside)
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const uint32_t r = pyramid::average<NODATA>(vec_get<T>(a, 2 * k), vec_get<T>(a, 2 * k + 1), vec_get<T>(b, 2 * k),
                                                            vec_get<T>(b, 2 * k + 1), true, has_y1, nodata);
                o[k / per] |= r << (bits * (k % per));
            }
        }
        *reinterpret_cast<uint2*>(d) = make_uint2(o[0], o[1]);
    } else {
        const int m = min(M, Wd - x0);
        for (int k = 0; k < m; ++k) d[k] = (T)pyramid::reduce_at<T, RESAMPLING, NODATA>(sp, row, Hs, Ws, y, x0 + k, nodata);
    }
}

template <class T, int RESAMPLING, bool NODATA>
static int launch_level(const T* src, int64_t row, int64_t plane, int C, int Hs, int Ws, T* dst, uint32_t nodata, hipStream_t s)
{
    constexpr int M = 8 / (int)sizeof(T);
    const int Hd = pyramid::half_up(Hs), Wd = pyramid::half_up(Ws);
    const int vpr = (Wd + M - 1) / M;
    const int64_t items = (int64_t)Hd * vpr;      // at most 2^29 + 2^19
    const dim3 grid((unsigned)((items + PT - 1) / PT), (unsigned)C);
    k_pyr_reduce<T, RESAMPLING, NODATA><<<grid, PT, 0, s>>>(src, row, plane, Hs, Ws, dst, Hd, Wd, vpr, nodata);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

template <class T>
static int build_levels(const lbdrn_pyr_desc& d, const T* src, int levels, unsigned char* out, hipStream_t s)
{
    const T* from = src;
    int64_t row = d.row_pitch, plane = d.plane_pitch;
    int Hs = d.H, Ws = d.W;
    for (int k = 1; k <= levels; ++k) {
        T* to = reinterpret_cast<T*>(out + pyramid::level_offset(d.C, d.H, d.W, k, (int)sizeof(T)));
        int rc;
        if (d.resampling == pyramid::NEAREST) rc = launch_level<T, pyramid::NEAREST, false>(from, row, plane, d.C, Hs, Ws, to, d.nodata, s);
        else if (d.has_nodata) rc = launch_level<T, pyramid::AVERAGE, true>(from, row, plane, d.C, Hs, Ws, to, d.nodata, s);
        else rc = launch_level<T, pyramid::AVERAGE, false>(from, row, plane, d.C, Hs, Ws, to, d.nodata, s);
        if (rc) return rc;
        Hs = pyramid::half_up(Hs);
        Ws = pyramid::half_up(Ws);
        from = to;
        row = Ws;
        plane = (int64_t)Hs * Ws;
    }
    return 0;
}

// the checks of a descriptor that the size functions and the build share
static int check_desc(const lbdrn_pyr_desc* d, const char* who)
{
    LBDRN_REQUIRE(d, "%s: null descriptor", who);
    LBDRN_REQUIRE(pyramid::geom_ok(d->C, d->H, d->W), "%s: geometry %d x %d x %d is out of range", who, d->C, d->H, d->W);
    LBDRN_REQUIRE(d->bits >= 1 && d->bits <= 32, "%s: %d-bit samples are out of range", who, d->bits);
    return 0;
}

static int sample_bytes(const lbdrn_pyr_desc& d) { return (d.bits + 7) / 8; }

static int pyr_build(const lbdrn_pyr_desc* d, const void* src, int levels, void* out, size_t out_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(d && src && out, "lbdrn_pyr_build: null pointer");
    if (int rc = check_desc(d, "lbdrn_pyr_build")) return rc;
    LBDRN_REQUIRE(d->row_pitch >= d->W, "lbdrn_pyr_build: row pitch %lld is below the width %d", (long long)d->row_pitch, d->W);
    LBDRN_REQUIRE(d->plane_pitch >= 0, "lbdrn_pyr_build: negative plane pitch");
    LBDRN_REQUIRE(d->has_nodata == 0 || d->has_nodata == 1, "lbdrn_pyr_build: has_nodata = %d: 0 or 1", d->has_nodata);
    LBDRN_REQUIRE(!d->has_nodata || d->bits == 32 || d->nodata < (1u << d->bits), "lbdrn_pyr_build: nodata = %u is no %d-bit sample",
                  d->nodata, d->bits);
    LBDRN_REQUIRE(levels >= 1 && levels <= pyramid::max_levels(d->H, d->W),
                  "lbdrn_pyr_build: levels = %d: a %d x %d raster has 1 .. %d (the source of a further one would be 1 x 1)", levels, d->H,
                  d->W, pyramid::max_levels(d->H, d->W));
    const int sb = sample_bytes(*d);
    LBDRN_REQUIRE(((uintptr_t)src | (uintptr_t)out) % (uintptr_t)sb == 0, "lbdrn_pyr_build: src or out is not aligned to a sample");
    const size_t need = pyramid::output_bytes(d->C, d->H, d->W, levels, sb);
    LBDRN_REQUIRE(out_bytes >= need, "lbdrn_pyr_build: out holds %zu bytes, %d levels need %zu", out_bytes, levels, need);
    if (d->bits != 8 && d->bits != 16) {
        set_error("lbdrn_pyr_build: %d-bit samples: unsigned 8 and 16 bits are reduced", d->bits);
        return LBDRN_E_UNSUPPORTED;
    }
    if (d->resampling != pyramid::AVERAGE && d->resampling != pyramid::NEAREST) {
        set_error("lbdrn_pyr_build: resampling %d: average (0) and nearest (1) are built", d->resampling);
        return LBDRN_E_UNSUPPORTED;
    }
    if (d->bits == 8) return build_levels<uint8_t>(*d, (const uint8_t*)src, levels, (unsigned char*)out, s);
    return build_levels<uint16_t>(*d, (const uint16_t*)src, levels, (unsigned char*)out, s);
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_pyr_last_error(void) { return lbdrn::last_error(); }
int lbdrn_pyr_abi_version(void) { return LBDRN_PYR_ABI_VERSION; }

int lbdrn_pyr_level_count(int32_t H, int32_t W, int32_t stop)
{
    LBDRN_REQUIRE(H >= 1 && W >= 1 && stop >= 1, "lbdrn_pyr_level_count: H = %d, W = %d, stop = %d: all at least 1", H, W, stop);
    return pyramid::auto_levels(H, W, stop);
}

int lbdrn_pyr_level_size(int32_t H, int32_t W, int32_t k, int32_t* Hk, int32_t* Wk)
{
    LBDRN_REQUIRE(Hk && Wk, "lbdrn_pyr_level_size: null pointer");
    LBDRN_REQUIRE(H >= 1 && W >= 1 && k >= 0 && k <= pyramid::max_levels(H, W), "lbdrn_pyr_level_size: a %d x %d raster has no level %d", H, W, k);
    int h, w;
    pyramid::level_size(H, W, k, &h, &w);
    *Hk = h;
    *Wk = w;
    return 0;
}

size_t lbdrn_pyr_level_offset(const lbdrn_pyr_desc* desc, int32_t k)
{
    if (lbdrn::check_desc(desc, "lbdrn_pyr_level_offset") || k < 1 || k > pyramid::max_levels(desc->H, desc->W)) return 0;
    return pyramid::level_offset(desc->C, desc->H, desc->W, k, lbdrn::sample_bytes(*desc));
}

size_t lbdrn_pyr_output_bytes(const lbdrn_pyr_desc* desc, int32_t levels)
{
    if (lbdrn::check_desc(desc, "lbdrn_pyr_output_bytes") || levels < 1 || levels > pyramid::max_levels(desc->H, desc->W)) return 0;
    return pyramid::output_bytes(desc->C, desc->H, desc->W, levels, lbdrn::sample_bytes(*desc));
}

int lbdrn_pyr_build(const lbdrn_pyr_desc* desc, const void* src, int32_t levels, void* out, size_t out_bytes, void* stream)
{
    return lbdrn::pyr_build(desc, src, levels, out, out_bytes, (hipStream_t)stream);
}

}  // extern "C"
